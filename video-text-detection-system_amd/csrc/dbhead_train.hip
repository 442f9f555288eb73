// DB head training (text_detector.py:58-86 DBHead, both branches, BatchNorm in train or eval mode), forward and backward, over a frozen
// trunk / FPN: the caller hands in P2 as "padded features" (ring-padded NHWC fp16 [n][H+2][W+2][256], include/vtd.h).
//
// Forward (M1 = n H W, M2 = 4 M1; channel c of a 128-wide tensor is branch c / 64, channel c % 64):
//   pack_weights     torch's fp32 parameters -> fp16 GEMM panels, on the device, every call (an optimizer step needs no re-pack)
//   conv 3x3         both branches as ONE N = 128 implicit GEMM (conv_igemm.hip, K = 2304) -> y1 fp32 [M1][128] (pre-BN)
//   stats            per-workgroup fp64 (count, mean, M2) partials, Chan's combination in a fixed order; running-stat update
//   bn_relu          a1 = relu(bn1(y1)) as an fp16 pair hi + lo [M1][2 branches][hi 64 | lo 64] (saved: the ConvT1 operand)
//   ConvT1           per branch a K = 128 (= hi and lo against the same weights), N = 256 GEMM with the pixel-shuffle store
//                    (conv_igemm.hip) -> z fp16 [M2][128] (pre-BN)
// y1 and a1 carry more than fp16, and z is stored CENTRED: BN2 normalises z = W1 a1 + b1, whose mean is large against its spread
// (a1 >= 0), and fp16 rounding of a1, y1 or of z itself moved the parameter gradients by ~1e-2 relative at small batches.  The ConvT1
// GEMM's bias is b1 - shift, every reader of z adds shift back (fp32), with shift[c] = b1 + mean over taps of W1 E[a1] and E[a1] the
// mean of relu(N(beta1, gamma1^2)) (a good estimate of z's channel mean; any shift is exact, a good one keeps z's fp16 rounding small).
//   stats            as above for BN2
//   convt2_sigmoid   a2 = relu(bn2(z)), ConvT(64 -> 1) + sigmoid, the two fp32 maps (N = 4: a per-pixel dot product, HBM-bound)
// Backward, g = upstream map gradients, s = the maps:
//   bwd_reduce<2>    dlogit = g s (1 - s), dz' = relu'(.) W2 dlogit; ConvT2 weight / bias gradients, sum dz', sum dz' x2^, max-abs bounds
//   bwd_finish<2>    BN2 gamma / beta gradients, the coefficients of BN2's backward, a power-of-two scale per branch
//   bwd_form<2>      dz = gamma2 invstd2 (dz' - mean dz' - x2^ mean(dz' x2^)) * scale -> fp16 [M2][128] (+ the ConvT1 bias gradient)
//   ConvT1 dgrad     per branch a 2x2 / stride-2 convolution of dz (conv_igemm.hip, K = 256) -> da1 fp32 [M1][128] (scaled)
//   wgrad<1>         ConvT1 weight gradient  sum_m a1[m]^T dz[pixel(m, tap)], split over M into slabs
//   bwd_reduce<1>, bwd_finish<1>, bwd_form<1>: the same three steps for BN1 -> dy1 fp16 [M1][128] (scaled) + the conv bias gradient
//   wgrad<0>         conv 3x3 weight gradient  dW[128][2304] = sum_m dy1[m]^T im2col(x)[m], split over M into slabs
//   wgrad_reduce     the slabs summed in slab order, the scale undone, written in torch's layout
// Input gradient (optional, a call of its own after the backward, on the same scratch; the steps above are untouched by it):
//   pack_dgrad       the 3x3 weights, taps rotated by 180 degrees and transposed, both branches along K: [256][9 * 128] fp16; the two
//                    branches' dy1 carry different power-of-two scales, so the branch with the larger one has the ratio folded into its
//                    weights (a power of two <= 1: exact) and one GEMM sums both at the common (smaller) scale
//   pad_dy1          dy1 [M1][128] -> ring-padded [n][H+2][W+2][128], ring zeroed (the layout a 3x3 window reads)
//   conv 3x3         dP2 = conv3x3^T(dy1) as ONE implicit GEMM (conv_igemm.hip, K = 1152, N = 256) -> fp32 [M1][256], scaled
// Every reduction has a grid that depends on the shape only and a fixed summation order, and no atomics: bitwise repeatable.
#include "vtd_common.h"
#include "wgrad_mfma.h"
#include "../../include/vtd.h"

#include <cstring>

#include "conv_kernels.h"

namespace {

constexpr int DHT_THREADS = 256;
constexpr int DHT_MAX_RED_BLOCKS = 1024;
constexpr int DHT_RED_VALS = 8;          // per channel and workgroup partial of the backward reductions
constexpr float DHT_SCALE_TARGET = 16384.0f;  // scaled operands stay below 2^14 (fp16 max 65504)

struct Branches {
    vtd_dbhead_branch b[2];
};

__host__ __device__ inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// reduction grids: a function of the row count only
inline int red_blocks(int64_t rows) {
    int64_t g = (rows + 511) / 512;
    return (int)(g < 1 ? 1 : g > DHT_MAX_RED_BLOCKS ? DHT_MAX_RED_BLOCKS : g);
}
inline int64_t rows_per_block(int64_t rows, int g) { return (rows + g - 1) / g; }

// weight-gradient slabs (split over M)
inline int wgrad_slabs(int64_t rows, int mode) {
    const int64_t per = mode == 0 ? 8192 : 4096, cap = mode == 0 ? 64 : 256;
    int64_t s = (rows + per - 1) / per;
    return (int)(s < 1 ? 1 : s > cap ? cap : s);
}
inline int64_t slab_rows(int64_t rows, int s) { return (rows_per_block(rows, s) + WG_KC - 1) / WG_KC * WG_KC; }

// ---- workspace layout (one function for the size query and every call) ----------------------------------------------------------------
struct FwdLayout {
    int64_t y1, a1, z, w3, wt1, wt1d, b3, bt1, zero, stat, part, total;
};
struct BwdLayout {
    int64_t dz, da1, dy1, coef2, coef1, part, bpart, slab, total;
};

// the input gradient's scratch, behind the backward's (mode 2 of the size query)
struct DgradLayout {
    int64_t dy1p, wd3, zero, total;
};

FwdLayout fwd_layout(int n, int H, int W) {
    FwdLayout L;
    const int64_t M1 = (int64_t)n * H * W, M2 = 4 * M1;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t r = o; o += align256(bytes); return r; };
    L.y1 = take(M1 * 128 * 4);
    L.a1 = take(M1 * 256 * 2);
    L.z = take(M2 * 128 * 2);
    L.w3 = take((int64_t)128 * 2304 * 2);
    L.wt1 = take((int64_t)2 * 256 * 128 * 2);
    L.wt1d = take((int64_t)2 * 64 * 256 * 2);
    L.b3 = take(128 * 4);
    L.bt1 = take(2 * 256 * 4);
    L.zero = take(256 * 4);
    L.stat = take(5 * 128 * 4);      // mean1, invstd1, mean2, invstd2, z shift
    L.part = take((int64_t)DHT_MAX_RED_BLOCKS * 128 * 3 * 8);
    L.total = o;
    return L;
}

BwdLayout bwd_layout(int n, int H, int W) {
    BwdLayout L;
    const int64_t M1 = (int64_t)n * H * W, M2 = 4 * M1;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t r = o; o += align256(bytes); return r; };
    L.dz = take(M2 * 128 * 2);
    L.da1 = take(M1 * 128 * 4);
    L.dy1 = take(M1 * 128 * 2);
    L.coef2 = take((3 * 128 + 6) * 4);   // k[128], mean dz'[128], mean dz'x^[128], scale[2], 1/scale[2], live[2]
    L.coef1 = take((3 * 128 + 6) * 4);
    L.part = take((int64_t)DHT_MAX_RED_BLOCKS * 128 * DHT_RED_VALS * 8);
    L.bpart = take((int64_t)DHT_MAX_RED_BLOCKS * 128 * 8);
    const int64_t s0 = (int64_t)wgrad_slabs(M1, 0) * 128 * 2304 * 4, s1 = (int64_t)wgrad_slabs(M1, 1) * 2 * 64 * 256 * 4;
    L.slab = take(s0 > s1 ? s0 : s1);
    L.total = o;
    return L;
}

DgradLayout dgrad_layout(int n, int H, int W) {
    DgradLayout L;
    int64_t o = bwd_layout(n, H, W).total;
    auto take = [&](int64_t bytes) { const int64_t r = o; o += align256(bytes); return r; };
    L.dy1p = take((int64_t)n * (H + 2) * (W + 2) * 128 * 2);
    L.wd3 = take((int64_t)256 * 1152 * 2);
    L.zero = take(256 * 4);
    L.total = o;
    return L;
}

// ---- input / weight packing ---------------------------------------------------------------------------------------------------------

// NCHW [n][256][H][W] (fp32 or fp16) -> padded NHWC fp16, ring zeroed.  One thread = 8 channels of one padded pixel.
template <typename T>
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_pack_features_kernel(const T* x, int n, int H, int W, half_t* out) {
    const int Hp = H + 2, Wp = W + 2;
    const int64_t total = (int64_t)n * Hp * Wp * 32;
    const int64_t i = (int64_t)blockIdx.x * DHT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int xp = (int)(i % Wp);
    const int64_t r = i / Wp;
    const int c8 = (int)(r % 32);
    const int64_t r2 = r / 32;
    const int yp = (int)(r2 % Hp), img = (int)(r2 / Hp);
    half8 v;
    const int y = yp - 1, xx = xp - 1;
    const bool inside = y >= 0 && y < H && xx >= 0 && xx < W;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = inside ? (half_t)(float)x[(((int64_t)img * 256 + c8 * 8 + e) * H + y) * W + xx] : (half_t)0.f;
    *(half8*)(out + (((int64_t)img * Hp + yp) * Wp + xp) * 256 + c8 * 8) = v;
}

// fp32 torch parameters -> fp16 panels (and fp32 bias rows) in the layouts conv_igemm.hip reads:
//   w3   [128][2304]        row b*64+co, k = (ky*3+kx)*256 + ci          conv 3x3, both branches
//   wt1  [2][256][128]      row (ky*2+kx)*64 + co, k = ci and 64 + ci     ConvT1 forward (pixel-shuffle GEMM over a1 hi | lo)
//   wt1d [2][64][256]       row ci, k = (ky*2+kx)*64 + co                ConvT1 input gradient (2x2 / stride-2 convolution of dz)
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_pack_weights_kernel(Branches P, half_t* w3, half_t* wt1, half_t* wt1d, float* b3,
                                                                                float* bt1, float* zero) {
    const int i = blockIdx.x * DHT_THREADS + threadIdx.x;
    constexpr int N3 = 128 * 2304, NT = 2 * 64 * 64 * 4;
    if (i < N3) {
        const int p = i / 2304, k = i % 2304, b = p / 64, co = p % 64, tap = k / 256, ci = k % 256;
        w3[i] = (half_t)P.b[b].conv_w[(co * 256 + ci) * 9 + tap];
    } else if (i < N3 + NT) {
        const int j = i - N3;  // torch order: [b][ci][co][ky][kx]
        const int b = j / 16384, r = j % 16384, ci = r / 256, co = (r / 4) % 64, tap = r % 4;
        const half_t h = (half_t)P.b[b].ct1_w[r];
        wt1[((int64_t)b * 256 + tap * 64 + co) * 128 + ci] = h;
        wt1[((int64_t)b * 256 + tap * 64 + co) * 128 + 64 + ci] = h;
        wt1d[((int64_t)b * 64 + ci) * 256 + tap * 64 + co] = h;
    } else if (i < N3 + NT + 128) {
        const int p = i - N3 - NT;
        b3[p] = P.b[p / 64].conv_b[p % 64];
    } else if (i < N3 + NT + 128 + 512) {
        const int q = i - N3 - NT - 128;
        bt1[q] = P.b[q / 256].ct1_b[q % 64];
    } else if (i < N3 + NT + 128 + 512 + 256) {
        zero[i - N3 - NT - 128 - 512] = 0.f;
    }
}
constexpr int PACK_W_ITEMS = 128 * 2304 + 2 * 64 * 64 * 4 + 128 + 512 + 256;

// ---- BatchNorm statistics --------------------------------------------------------------------------------------------------------
// y: [rows][128] fp32 (y1) or fp16 (z).  Thread (channel pair c2 = t % 64, row lane r = t / 64); fp64 sums of y and y^2 over the rows of one workgroup,
// the four row lanes added in order, then (count, mean, M2) per channel: part[g][c][3].
template <typename T>
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_stats_partial_kernel(const T* y, int64_t rows, int64_t per, const float* shift,
                                                                                 double* part) {
    const int t = threadIdx.x, c2 = t & 63, r = t >> 6;
    const float sh0 = shift ? shift[2 * c2] : 0.f, sh1 = shift ? shift[2 * c2 + 1] : 0.f;
    const int64_t m0 = (int64_t)blockIdx.x * per, m1 = m0 + per < rows ? m0 + per : rows;
    double s0 = 0.0, s1 = 0.0, q0 = 0.0, q1 = 0.0;
    for (int64_t m = m0 + r; m < m1; m += 4) {
        const double a = (double)((float)y[m * 128 + 2 * c2] + sh0), b = (double)((float)y[m * 128 + 2 * c2 + 1] + sh1);
        s0 += a; q0 += a * a; s1 += b; q1 += b * b;
    }
    __shared__ double sh[4][64][4];
    sh[r][c2][0] = s0; sh[r][c2][1] = q0; sh[r][c2][2] = s1; sh[r][c2][3] = q1;
    __syncthreads();
    if (t < 128) {
        const int cp = t >> 1, e = t & 1;
        double s = 0.0, q = 0.0;
        for (int k = 0; k < 4; ++k) { s += sh[k][cp][2 * e]; q += sh[k][cp][2 * e + 1]; }
        const double cnt = (double)(m1 > m0 ? m1 - m0 : 0);
        const double mean = cnt > 0 ? s / cnt : 0.0;
        const double m2 = cnt > 0 ? fmax(q - s * mean, 0.0) : 0.0;
        double* o = part + ((int64_t)blockIdx.x * 128 + 2 * cp + e) * 3;
        o[0] = cnt; o[1] = mean; o[2] = m2;
    }
}

// One thread per channel: Chan's pairwise combination of the partials in workgroup order (fp64), then mean / invstd for the
// normalisation and, in training mode, torch's running-stat update.  layer: 0 = BN1, 1 = BN2.
__global__ __launch_bounds__(128) void dbhead_train_stats_finish_kernel(const double* part, int G, Branches P, int layer, int training,
                                                                        float momentum, float eps, float* stat, float* stats_out) {
    const int c = threadIdx.x, b = c >> 6, cc = c & 63;
    float* rm = layer ? P.b[b].bn2_mean : P.b[b].bn1_mean;
    float* rv = layer ? P.b[b].bn2_var : P.b[b].bn1_var;
    double mean, var;
    if (training) {
        double n = 0.0, mu = 0.0, m2 = 0.0;
        for (int g = 0; g < G; ++g) {
            const double* q = part + ((int64_t)g * 128 + c) * 3;
            const double nb = q[0];
            if (nb <= 0.0) continue;
            const double tot = n + nb, d = q[1] - mu;
            mu += d * (nb / tot);
            m2 += q[2] + d * d * (n * nb / tot);
            n = tot;
        }
        mean = mu;
        var = m2 / n;
        const double unbiased = n > 1.0 ? m2 / (n - 1.0) : m2;
        rm[cc] = (float)((1.0 - (double)momentum) * (double)rm[cc] + (double)momentum * mean);
        rv[cc] = (float)((1.0 - (double)momentum) * (double)rv[cc] + (double)momentum * unbiased);
    } else {
        mean = (double)rm[cc];
        var = (double)rv[cc];
    }
    stat[c] = (float)mean;
    stat[128 + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (stats_out) {
        stats_out[layer * 256 + c] = (float)mean;
        stats_out[layer * 256 + 128 + c] = (float)var;
    }
}

// a1 = relu(bn1(y1)) as the fp16 pair hi = fp16(a1), lo = fp16(a1 - hi); one thread = 8 channels of one row
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_bn_relu_kernel(const float* y, int64_t rows, Branches P, const float* stat, half_t* a) {
    __shared__ float mu[128], is[128], gm[128], bt[128];
    if (threadIdx.x < 128) {
        const int c = threadIdx.x, b = c >> 6, cc = c & 63;
        mu[c] = stat[c]; is[c] = stat[128 + c]; gm[c] = P.b[b].bn1_w[cc]; bt[c] = P.b[b].bn1_b[cc];
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * DHT_THREADS + threadIdx.x;
    if (i >= rows * 16) return;
    const int c0 = (int)(i & 15) * 8;
    const int64_t m = i >> 4;
    const floatx4 v0 = *(const floatx4*)(y + i * 8), v1 = *(const floatx4*)(y + i * 8 + 4);
    half8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        float t = ((e < 4 ? v0[e] : v1[e - 4]) - mu[c]) * is[c] * gm[c] + bt[c];   // aten batch_norm: (x - mean) * invstd * weight + bias
        t = t > 0.f ? t : 0.f;
        hi[e] = (half_t)t;
        lo[e] = (half_t)(t - (float)hi[e]);
    }
    half_t* dst = a + m * 256 + (c0 >> 6) * 128 + (c0 & 63);
    *(half8*)dst = hi;
    *(half8*)(dst + 64) = lo;
}

// z shift (see the top of this file) and the ConvT1 GEMM bias b1 - shift; one thread per channel
__global__ __launch_bounds__(128) void dbhead_train_zshift_kernel(Branches P, float* shift, float* bt1) {
    const int c = threadIdx.x, b = c >> 6, co = c & 63;
    double acc = 0.0;
    for (int ci = 0; ci < 64; ++ci) {
        const double g = fabs((double)P.b[b].bn1_w[ci]), be = (double)P.b[b].bn1_b[ci];
        const double ea = g < 1e-12 ? fmax(be, 0.0) : be * 0.5 * erfc(-be / g * 0.70710678118654752) + g * exp(-0.5 * (be / g) * (be / g)) * 0.39894228040143268;
        const float* w = P.b[b].ct1_w + (ci * 64 + co) * 4;
        acc += ea * 0.25 * ((double)w[0] + (double)w[1] + (double)w[2] + (double)w[3]);
    }
    const float b1 = P.b[b].ct1_b[co];
    const float sh = (float)((double)b1 + acc);
    shift[c] = sh;
    for (int tap = 0; tap < 4; ++tap) bt1[b * 256 + tap * 64 + co] = b1 - sh;
}

// ConvT(64 -> 1, k2 s2) + sigmoid on a2 = relu(bn2(z)).  One thread = one (z pixel, branch): 64 channels in, a 2x2 patch of one map out.
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_convt2_sigmoid_kernel(const half_t* z, int n, int H2, int W2, Branches P, const float* stat,
                                                                                  float* prob, float* thresh) {
    __shared__ float mu[128], is[128], gm[128], bt[128], w2[128][4], b2[2];
    if (threadIdx.x < 128) {
        const int c = threadIdx.x, b = c >> 6, cc = c & 63;
        mu[c] = stat[256 + c] - stat[512 + c]; is[c] = stat[384 + c]; gm[c] = P.b[b].bn2_w[cc]; bt[c] = P.b[b].bn2_b[cc];
#pragma unroll
        for (int q = 0; q < 4; ++q) w2[c][q] = P.b[b].ct2_w[cc * 4 + q];
        if (cc == 0) b2[b] = P.b[b].ct2_b[0];
    }
    __syncthreads();
    const int64_t M2 = (int64_t)n * H2 * W2;
    const int64_t i = (int64_t)blockIdx.x * DHT_THREADS + threadIdx.x;
    if (i >= 2 * M2) return;
    const int b = (int)(i & 1);
    const int64_t m = i >> 1;
    const half_t* src = z + m * 128 + b * 64;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const half8 v = *(const half8*)(src + 8 * k);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = b * 64 + 8 * k + e;
            float t = ((float)v[e] - mu[c]) * is[c] * gm[c] + bt[c];
            t = t > 0.f ? t : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] += t * w2[c][q];
        }
    }
    const int x2 = (int)(m % W2);
    const int64_t r = m / W2;
    const int y2 = (int)(r % H2), img = (int)(r / H2);
    float* dst = (b ? thresh : prob) + ((int64_t)img * 2 * H2 + 2 * y2) * 2 * W2 + 2 * x2;
    float s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = 1.f / (1.f + expf(-(o[q] + b2[b])));
    *(float2*)dst = make_float2(s[0], s[1]);
    *(float2*)(dst + 2 * W2) = make_float2(s[2], s[3]);
}

// ---- backward reductions ---------------------------------------------------------------------------------------------------------
// LEVEL 2: tensor z [M2][128] fp16, gradient formed from the maps; LEVEL 1: tensor y1 [M1][128] fp16, gradient da1 (fp32, scaled by
// the BN2 pass's scale).  Both: x^ = (v - mean) invstd, pre = gamma x^ + beta, d' = d * (pre > 0).
struct BwdArgs {
    const half_t* vh;           // LEVEL 2: z [M2][128] fp16
    const float* vf;            // LEVEL 1: y1 [M1][128] fp32
    const float* zshift;        // LEVEL 2: added to z (see the top of this file)
    const float* stat;          // mean[128], invstd[128] of this layer
    const float* da1;           // LEVEL 1: [M1][128] scaled input gradient
    const float* inv_sc_in;     // LEVEL 1: 1 / scale of da1 per branch (coef2 + 386)
    const float* s0; const float* s1;   // LEVEL 2: the maps
    const float* g0; const float* g1;   // LEVEL 2: their upstream gradients (null = 0)
    int n, H2, W2;              // LEVEL 2 geometry (z pixels)
    int64_t rows, per;
};

struct PixGrad {
    float dl[4];
};

template <int LEVEL>
__device__ __forceinline__ void load_pix_grad(const BwdArgs& A, int b, int64_t m, PixGrad& pg) {
    const int x2 = (int)(m % A.W2);
    const int64_t r = m / A.W2;
    const int y2 = (int)(r % A.H2), img = (int)(r / A.H2);
    const int64_t o = ((int64_t)img * 2 * A.H2 + 2 * y2) * 2 * A.W2 + 2 * x2;
    const float* s = b ? A.s1 : A.s0;
    const float* g = b ? A.g1 : A.g0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t oo = o + (q >> 1) * 2 * A.W2 + (q & 1);
        const float sv = s[oo];
        const float gv = g ? g[oo] : 0.f;
        pg.dl[q] = gv * (1.f - sv) * sv;   // aten sigmoid_backward: grad * (1 - y) * y
    }
}

// per-element gradient d' (after the ReLU mask) and x^, shared by the reduce and form passes so both see the same values
template <int LEVEL>
__device__ __forceinline__ void elem_grad(const BwdArgs& A, const float* w2c /*[4], LEVEL 2*/, const PixGrad& pg, float v, float mu, float is, float gm,
                                          float bt, int64_t m, int c, float& dprime, float& xh, float& act) {
    xh = (v - mu) * is;
    const float pre = (v - mu) * is * gm + bt;
    act = pre > 0.f ? pre : 0.f;
    float d;
    if constexpr (LEVEL == 2) {
        d = w2c[0] * pg.dl[0] + w2c[1] * pg.dl[1] + w2c[2] * pg.dl[2] + w2c[3] * pg.dl[3];
    } else {
        d = A.da1[m * 128 + c] * A.inv_sc_in[c >> 6];
    }
    dprime = pre > 0.f ? d : 0.f;
}

// part[g][c][8]: LEVEL 2 = {dW2[0..3], sum d', sum d' x^, max|d'|, max|x^|}, LEVEL 1 = {sum d', sum d' x^, max|d'|, max|x^|, 0...};
// bpart[g][2] (LEVEL 2): the ConvT2 bias gradient partial per branch (sum over pixels of sum_q dlogit)
template <int LEVEL>
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_bwd_reduce_kernel(const BwdArgs A, Branches P, double* part, double* bpart) {
    __shared__ float mu[128], is[128], gm[128], bt[128], w2[128][4];
    const int t = threadIdx.x;
    if (t < 128) {
        const int b = t >> 6, cc = t & 63;
        mu[t] = A.stat[t]; is[t] = A.stat[128 + t];
        gm[t] = LEVEL == 2 ? P.b[b].bn2_w[cc] : P.b[b].bn1_w[cc];
        bt[t] = LEVEL == 2 ? P.b[b].bn2_b[cc] : P.b[b].bn1_b[cc];
#pragma unroll
        for (int q = 0; q < 4; ++q) w2[t][q] = LEVEL == 2 ? P.b[b].ct2_w[cc * 4 + q] : 0.f;
    }
    __syncthreads();
    const int c2 = t & 63, r = t >> 6, b = c2 >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * A.per, m1 = m0 + A.per < A.rows ? m0 + A.per : A.rows;
    double acc[2][DHT_RED_VALS];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int k = 0; k < DHT_RED_VALS; ++k) acc[e][k] = 0.0;
    double bsum = 0.0;
    for (int64_t m = m0 + r; m < m1; m += 4) {
        PixGrad pg;
        if constexpr (LEVEL == 2) {
            load_pix_grad<LEVEL>(A, b, m, pg);
            if ((c2 & 31) == 0) bsum += (double)pg.dl[0] + (double)pg.dl[1] + (double)pg.dl[2] + (double)pg.dl[3];
        }
        float v[2];
        if constexpr (LEVEL == 2) {
            const half2v h = *(const half2v*)(A.vh + m * 128 + 2 * c2);
            v[0] = (float)h[0] + A.zshift[2 * c2]; v[1] = (float)h[1] + A.zshift[2 * c2 + 1];
        } else {
            const float2 f = *(const float2*)(A.vf + m * 128 + 2 * c2);
            v[0] = f.x; v[1] = f.y;
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = 2 * c2 + e;
            float dp, xh, act;
            elem_grad<LEVEL>(A, w2[c], pg, v[e], mu[c], is[c], gm[c], bt[c], m, c, dp, xh, act);
            double* a = acc[e];
            int k = 0;
            if constexpr (LEVEL == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] += (double)act * (double)pg.dl[q];
                k = 4;
            }
            a[k] += (double)dp;
            a[k + 1] += (double)dp * (double)xh;
            a[k + 2] = fmax(a[k + 2], (double)fabsf(dp));
            a[k + 3] = fmax(a[k + 3], (double)fabsf(xh));
        }
    }
    __shared__ double sh[4][128][DHT_RED_VALS];
    __shared__ double shb[4][2];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int k = 0; k < DHT_RED_VALS; ++k) sh[r][2 * c2 + e][k] = acc[e][k];
    if ((c2 & 31) == 0) shb[r][b] = bsum;
    __syncthreads();
    const int nsum = LEVEL == 2 ? 6 : 2;   // the first nsum values are sums, the next two maxima
    for (int j = t; j < 128 * DHT_RED_VALS; j += DHT_THREADS) {
        const int c = j / DHT_RED_VALS, k = j % DHT_RED_VALS;
        double s = sh[0][c][k];
        for (int rr = 1; rr < 4; ++rr) s = k < nsum ? s + sh[rr][c][k] : fmax(s, sh[rr][c][k]);
        part[((int64_t)blockIdx.x * 128 + c) * DHT_RED_VALS + k] = s;
    }
    if (LEVEL == 2 && t < 2) bpart[(int64_t)blockIdx.x * 2 + t] = shb[0][t] + shb[1][t] + shb[2][t] + shb[3][t];
}

// One thread per channel: partials in workgroup order; gradients of this BN's gamma / beta (and of ConvT2 at LEVEL 2); the coefficients
// of the BN backward (training: dy = k (d' - A - x^ B) with k = gamma invstd, A = mean d', B = mean d' x^; eval: A = B = 0); a
// power-of-two scale per branch from the bound |k| (max|d'| + |A| + max|x^| |B|) >= max |dy|.
// coef: k[128], A[128], B[128], scale[2], 1/scale[2], live[2] (1 = the branch's bound is finite and not zero: its scale means something)
template <int LEVEL>
__global__ __launch_bounds__(128) void dbhead_train_bwd_finish_kernel(const double* part, const double* bpart, int G, int64_t rows, int training,
                                                                      Branches P, Branches Gr, const float* stat, float* coef) {
    const int c = threadIdx.x, b = c >> 6, cc = c & 63;
    const int nsum = LEVEL == 2 ? 6 : 2;
    double v[DHT_RED_VALS];
    for (int k = 0; k < DHT_RED_VALS; ++k) v[k] = part[(int64_t)c * DHT_RED_VALS + k];
    for (int g = 1; g < G; ++g)
        for (int k = 0; k < DHT_RED_VALS; ++k) {
            const double x = part[((int64_t)g * 128 + c) * DHT_RED_VALS + k];
            v[k] = k < nsum ? v[k] + x : fmax(v[k], x);
        }
    const int o = LEVEL == 2 ? 4 : 0;
    const double sd = v[o], sdx = v[o + 1], mxd = v[o + 2], mxx = v[o + 3];
    if (LEVEL == 2) {
        for (int q = 0; q < 4; ++q) Gr.b[b].ct2_w[cc * 4 + q] = (float)v[q];
        if (cc == 0) {
            double s = 0.0;
            for (int g = 0; g < G; ++g) s += bpart[(int64_t)g * 2 + b];
            Gr.b[b].ct2_b[0] = (float)s;
        }
        Gr.b[b].bn2_w[cc] = (float)sdx;
        Gr.b[b].bn2_b[cc] = (float)sd;
    } else {
        Gr.b[b].bn1_w[cc] = (float)sdx;
        Gr.b[b].bn1_b[cc] = (float)sd;
    }
    const float gm = LEVEL == 2 ? P.b[b].bn2_w[cc] : P.b[b].bn1_w[cc];
    const double k = (double)gm * (double)stat[128 + c];
    const double Am = training ? sd / (double)rows : 0.0, Bm = training ? sdx / (double)rows : 0.0;
    coef[c] = (float)k;
    coef[128 + c] = (float)Am;
    coef[256 + c] = (float)Bm;
    __shared__ double bound[128];
    bound[c] = fabs(k) * (mxd + fabs(Am) + mxx * fabs(Bm));
    __syncthreads();
    if (c < 2) {
        double mx = 0.0;
        for (int j = 0; j < 64; ++j) mx = fmax(mx, bound[c * 64 + j]);
        int e = 0;
        if (mx > 0.0 && isfinite(mx)) {
            e = (int)floor(log2((double)DHT_SCALE_TARGET / mx));
            e = e < -100 ? -100 : e > 100 ? 100 : e;
        }
        coef[384 + c] = ldexpf(1.0f, e);
        coef[386 + c] = ldexpf(1.0f, -e);
        coef[388 + c] = (mx > 0.0 && isfinite(mx)) ? 1.f : 0.f;
    }
}

// dy = k (d' - A - x^ B), times the branch's scale, as fp16 [rows][128]; bpart[g][128] = fp64 sum of dy (unscaled) per channel: the
// gradient of the bias in front of this BatchNorm
template <int LEVEL>
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_bwd_form_kernel(const BwdArgs A, Branches P, const float* coef, half_t* out, double* bpart) {
    __shared__ float mu[128], is[128], gm[128], bt[128], w2[128][4], kk[128], am[128], bm[128], sc[2];
    const int t = threadIdx.x;
    if (t < 128) {
        const int b = t >> 6, cc = t & 63;
        mu[t] = A.stat[t]; is[t] = A.stat[128 + t];
        gm[t] = LEVEL == 2 ? P.b[b].bn2_w[cc] : P.b[b].bn1_w[cc];
        bt[t] = LEVEL == 2 ? P.b[b].bn2_b[cc] : P.b[b].bn1_b[cc];
#pragma unroll
        for (int q = 0; q < 4; ++q) w2[t][q] = LEVEL == 2 ? P.b[b].ct2_w[cc * 4 + q] : 0.f;
        kk[t] = coef[t]; am[t] = coef[128 + t]; bm[t] = coef[256 + t];
        if (t < 2) sc[t] = coef[384 + t];
    }
    __syncthreads();
    const int c2 = t & 63, r = t >> 6, b = c2 >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * A.per, m1 = m0 + A.per < A.rows ? m0 + A.per : A.rows;
    double s[2] = {0.0, 0.0};
    for (int64_t m = m0 + r; m < m1; m += 4) {
        PixGrad pg;
        if constexpr (LEVEL == 2) load_pix_grad<LEVEL>(A, b, m, pg);
        float v[2];
        if constexpr (LEVEL == 2) {
            const half2v h = *(const half2v*)(A.vh + m * 128 + 2 * c2);
            v[0] = (float)h[0] + A.zshift[2 * c2]; v[1] = (float)h[1] + A.zshift[2 * c2 + 1];
        } else {
            const float2 f = *(const float2*)(A.vf + m * 128 + 2 * c2);
            v[0] = f.x; v[1] = f.y;
        }
        half2v o;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = 2 * c2 + e;
            float dp, xh, act;
            elem_grad<LEVEL>(A, w2[c], pg, v[e], mu[c], is[c], gm[c], bt[c], m, c, dp, xh, act);
            const float dy = kk[c] * (dp - am[c] - xh * bm[c]);
            s[e] += (double)dy;
            o[e] = (half_t)(dy * sc[b]);
        }
        *(half2v*)(out + m * 128 + 2 * c2) = o;
    }
    __shared__ double sh[4][128];
    sh[r][2 * c2] = s[0];
    sh[r][2 * c2 + 1] = s[1];
    __syncthreads();
    if (t < 128) bpart[(int64_t)blockIdx.x * 128 + t] = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
}

// bias gradient = sum of the partials in workgroup order.  which: 0 = conv_b (LEVEL 1), 1 = ct1_b (LEVEL 2)
__global__ __launch_bounds__(128) void dbhead_train_bias_finish_kernel(const double* bpart, int G, Branches Gr, int which) {
    const int c = threadIdx.x, b = c >> 6, cc = c & 63;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += bpart[(int64_t)g * 128 + c];
    (which ? Gr.b[b].ct1_b : Gr.b[b].conv_b)[cc] = (float)s;
}

// ---- weight gradients: the MFMA kernel is wgrad_mfma.h (shared with fpn_train.hip); MODE 0 = conv 3x3, MODE 1 = ConvT1 ----------------------
// slabs summed in slab order, scale undone per branch, written in torch's layout
template <int MODE>
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_wgrad_reduce_kernel(const float* slab, int S, const float* inv_sc, Branches Gr) {
    constexpr int NEL = MODE == 0 ? 128 * 2304 : 2 * 64 * 256;
    const int i = blockIdx.x * DHT_THREADS + threadIdx.x;
    if (i >= NEL) return;
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += (double)slab[(int64_t)k * NEL + i];
    if constexpr (MODE == 0) {
        const int p = i / 2304, q = i % 2304, b = p >> 6, co = p & 63, tap = q / 256, ci = q % 256;
        Gr.b[b].conv_w[(co * 256 + ci) * 9 + tap] = (float)(s * (double)inv_sc[b]);
    } else {
        const int b = i / 16384, r = i % 16384, ci = r / 256, q = r % 256, tap = q / 64, co = q % 64;
        Gr.b[b].ct1_w[(ci * 64 + co) * 4 + tap] = (float)(s * (double)inv_sc[b]);
    }
}

// ---- input gradient: dP2 = conv3x3^T(dy1) ---------------------------------------------------------------------------------------------
// wd3 [256][1152]: row ci, k = tap' * 128 + b * 64 + co holds w_b[co][ci][8 - tap'] (the window rotated by 180 degrees), rounded to fp16 as
// the forward packs it, times common / scale_b with common = the smaller of the live branches' dy1 scales (coef1 + 384): a power of two
// <= 1, exact unless the product falls below fp16's normal range -- which takes a ratio below ~2^-10, i.e. a branch whose whole gradient
// is below the other's fp16 rounding.  A branch that is not live (coef1 + 388: its dy1 is all zeros, or its bound is not finite) takes
// no part in the choice, and its weights are packed as zeros (0 x 0 = 0, 0 x inf = NaN as torch would give).  dscale = {common, 1 / common}.
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_pack_dgrad_weights_kernel(Branches P, const float* coef1, half_t* wd3, float* zero,
                                                                                      float* dscale) {
    const int i = blockIdx.x * DHT_THREADS + threadIdx.x;
    const float s0 = coef1[384], s1 = coef1[385];
    const bool l0 = coef1[388] != 0.f, l1 = coef1[389] != 0.f;
    const float common = l0 && l1 ? (s0 < s1 ? s0 : s1) : l0 ? s0 : l1 ? s1 : 1.f;
    if (i < 256 * 1152) {
        const int ci = i / 1152, k = i % 1152, tap = k / 128, c = k % 128, b = c >> 6, co = c & 63;
        const half_t h = (half_t)P.b[b].conv_w[(co * 256 + ci) * 9 + (8 - tap)];
        wd3[i] = (b ? l1 : l0) ? (half_t)((float)h * (common / (b ? s1 : s0))) : (half_t)0.f;
    } else if (i < 256 * 1152 + 256) {
        zero[i - 256 * 1152] = 0.f;
    } else if (i == 256 * 1152 + 256) {
        dscale[0] = common;
        dscale[1] = 1.0f / common;
    }
}
constexpr int PACK_DGRAD_ITEMS = 256 * 1152 + 256 + 1;

// dy1 [M1][128] fp16 -> ring-padded [n][H+2][W+2][128], ring zeroed.  One thread = 8 channels (16 bytes) of one padded pixel.
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_pad_dy1_kernel(const half_t* dy1, int n, int H, int W, half_t* out) {
    const int Hp = H + 2, Wp = W + 2;
    const int64_t i = (int64_t)blockIdx.x * DHT_THREADS + threadIdx.x;
    if (i >= (int64_t)n * Hp * Wp * 16) return;
    const int c8 = (int)(i & 15);
    const int64_t pp = i >> 4;
    const int xp = (int)(pp % Wp);
    const int64_t r = pp / Wp;
    const int yp = (int)(r % Hp), img = (int)(r / Hp);
    const int y = yp - 1, x = xp - 1;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (y >= 0 && y < H && x >= 0 && x < W) v = *(const half8*)(dy1 + (((int64_t)img * H + y) * W + x) * 128 + c8 * 8);
    *(half8*)(out + i * 8) = v;
}

// scaled NHWC fp32 [n][H][W][256] -> NCHW fp32 [n][256][H][W], the scale undone.  Workgroup = 64 pixels of one image x 64 channels through
// an LDS tile: 256-byte rows in, 256-byte rows out.
__global__ __launch_bounds__(DHT_THREADS) void dbhead_train_unpack_input_grad_kernel(const float* d, const float* dscale, int HW, float* out) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x, lane = t & 63, row = t >> 6;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, img = blockIdx.z;
    const float inv = dscale[1];
    for (int r = row; r < 64; r += 4) {
        const int p = p0 + r;
        tile[r][lane] = p < HW ? d[((int64_t)img * HW + p) * 256 + c0 + lane] * inv : 0.f;
    }
    __syncthreads();
    for (int r = row; r < 64; r += 4) {
        const int p = p0 + lane;
        if (p < HW) out[((int64_t)img * 256 + c0 + r) * HW + p] = tile[lane][r];
    }
}

inline unsigned blocks_for(int64_t items) { return (unsigned)((items + DHT_THREADS - 1) / DHT_THREADS); }

bool params_ok(const vtd_dbhead_params* p, bool need_stats) {
    if (!p) return false;
    for (int b = 0; b < 2; ++b) {
        const vtd_dbhead_branch& r = p->branch[b];
        const float* f[14] = {r.conv_w, r.conv_b, r.bn1_w, r.bn1_b, r.bn1_mean, r.bn1_var, r.ct1_w, r.ct1_b, r.bn2_w, r.bn2_b, r.bn2_mean, r.bn2_var,
                              r.ct2_w, r.ct2_b};
        for (int k = 0; k < 14; ++k) {
            const bool is_stat = k == 4 || k == 5 || k == 10 || k == 11;
            if (is_stat && !need_stats) continue;
            if (!f[k] || ((uintptr_t)f[k] & 3)) return false;
        }
    }
    return true;
}

ConvParams base_conv() {
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.k_hi_step = 32;
    p.stride = 1;
    return p;
}

}  // namespace

int64_t vtd_dbhead_ws_bytes(int n, int H, int W, int backward) {
    if (n <= 0 || H <= 0 || W <= 0 || (int64_t)n * H * W * 4 >= (1ll << 31)) return -2802;
    return backward == 2 ? dgrad_layout(n, H, W).total : backward ? bwd_layout(n, H, W).total : fwd_layout(n, H, W).total;
}

int vtd_launch_dbhead_pack(const void* x, int dtype, int n, int H, int W, void* feats, hipStream_t s) {
    if (!x || !feats || n <= 0 || H <= 0 || W <= 0 || (dtype != 0 && dtype != 1)) return -2802;
    if ((uintptr_t)feats & 15) return -2803;
    const int64_t items = (int64_t)n * (H + 2) * (W + 2) * 32;
    if (dtype == 0)
        hipLaunchKernelGGL(dbhead_train_pack_features_kernel<float>, dim3(blocks_for(items)), dim3(DHT_THREADS), 0, s, (const float*)x, n, H, W, (half_t*)feats);
    else
        hipLaunchKernelGGL(dbhead_train_pack_features_kernel<half_t>, dim3(blocks_for(items)), dim3(DHT_THREADS), 0, s, (const half_t*)x, n, H, W, (half_t*)feats);
    return -(int)hipGetLastError();
}

int vtd_launch_dbhead_forward(const void* feats, int n, int H, int W, const vtd_dbhead_params* params, int training, float momentum, float eps,
                              void* ws, float* prob, float* thresh, float* stats_out, hipStream_t s) {
    if (!feats || !ws || !prob || !thresh || !params_ok(params, true) || vtd_dbhead_ws_bytes(n, H, W, 0) < 0) return -2802;
    if (((uintptr_t)feats & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)prob & 7) || ((uintptr_t)thresh & 7) || ((uintptr_t)stats_out & 3)) return -2803;
    const FwdLayout L = fwd_layout(n, H, W);
    char* w = (char*)ws;
    float* y1 = (float*)(w + L.y1);
    half_t *a1 = (half_t*)(w + L.a1), *z = (half_t*)(w + L.z);
    half_t *w3 = (half_t*)(w + L.w3), *wt1 = (half_t*)(w + L.wt1), *wt1d = (half_t*)(w + L.wt1d);
    float *b3 = (float*)(w + L.b3), *bt1 = (float*)(w + L.bt1), *zero = (float*)(w + L.zero), *stat = (float*)(w + L.stat);
    double* part = (double*)(w + L.part);
    Branches P;
    P.b[0] = params->branch[0];
    P.b[1] = params->branch[1];
    const int64_t M1 = (int64_t)n * H * W, M2 = 4 * M1;
    int rc;
    hipLaunchKernelGGL(dbhead_train_pack_weights_kernel, dim3(blocks_for(PACK_W_ITEMS)), dim3(DHT_THREADS), 0, s, P, w3, wt1, wt1d, b3, bt1, zero);
    VTD_HIP_CHECK(hipGetLastError());
    {   // conv 3x3 256 -> 128 (both branches), bias, no activation: y1
        ConvParams c = base_conv();
        c.in = (const half_t*)feats; c.wgt = w3; c.bias = b3; c.out = y1; c.ldc = 128; c.flags = EPI_OUT_F32;
        c.cin_steps = 4; c.kw = 3; c.s_step = 256; c.r_step = (W + 2) * 256;
        c.M = (int)M1; c.K = 2304; c.cout = 128; c.cout_pad = 128; c.ho = H; c.wo = W;
        c.in_hp = H + 2; c.in_wp = W + 2; c.in_c = 256; c.in_y0 = 0; c.in_x0 = 0;
        if ((rc = vtd_launch_conv(c, -1, s))) return rc;
    }
    const int G1 = red_blocks(M1), G2 = red_blocks(M2);
    hipLaunchKernelGGL(dbhead_train_stats_partial_kernel<float>, dim3(G1), dim3(DHT_THREADS), 0, s, (const float*)y1, M1, rows_per_block(M1, G1),
                       (const float*)nullptr, part);
    hipLaunchKernelGGL(dbhead_train_stats_finish_kernel, dim3(1), dim3(128), 0, s, (const double*)part, G1, P, 0, training, momentum, eps, stat, stats_out);
    hipLaunchKernelGGL(dbhead_train_bn_relu_kernel, dim3(blocks_for(M1 * 16)), dim3(DHT_THREADS), 0, s, (const float*)y1, M1, P, (const float*)stat, a1);
    hipLaunchKernelGGL(dbhead_train_zshift_kernel, dim3(1), dim3(128), 0, s, P, stat + 512, bt1);
    VTD_HIP_CHECK(hipGetLastError());
    for (int b = 0; b < 2; ++b) {   // ConvT1 64 -> 64, k2 s2, bias: z (pixel-shuffle store into this branch's 64 channels)
        ConvParams c = base_conv();
        c.in = a1 + b * 128; c.wgt = wt1 + (int64_t)b * 256 * 128; c.bias = bt1 + b * 256; c.out = z + b * 64;
        c.cin_steps = 2; c.kw = 1; c.s_step = 0; c.r_step = 0;
        c.M = (int)M1; c.K = 128; c.cout = 256; c.cout_pad = 256; c.ho = H; c.wo = W;
        c.in_hp = H; c.in_wp = W; c.in_c = 256; c.in_y0 = 0; c.in_x0 = 0;
        c.out_hp = 2 * H; c.out_wp = 2 * W; c.out_c = 128; c.out_ring = 0;
        c.flags = EPI_PIXEL_SHUFFLE; c.ps_cout = 64;
        if ((rc = vtd_launch_conv(c, -1, s))) return rc;
    }
    hipLaunchKernelGGL(dbhead_train_stats_partial_kernel<half_t>, dim3(G2), dim3(DHT_THREADS), 0, s, (const half_t*)z, M2, rows_per_block(M2, G2),
                       (const float*)(stat + 512), part);
    hipLaunchKernelGGL(dbhead_train_stats_finish_kernel, dim3(1), dim3(128), 0, s, (const double*)part, G2, P, 1, training, momentum, eps, stat + 256,
                       stats_out);
    hipLaunchKernelGGL(dbhead_train_convt2_sigmoid_kernel, dim3(blocks_for(2 * M2)), dim3(DHT_THREADS), 0, s, (const half_t*)z, n, 2 * H, 2 * W, P,
                       (const float*)stat, prob, thresh);
    (void)zero;
    return -(int)hipGetLastError();
}

int vtd_launch_dbhead_backward(const void* feats, int n, int H, int W, const vtd_dbhead_params* params, int training, const void* ws,
                               const float* prob, const float* thresh, const float* gprob, const float* gthresh, const vtd_dbhead_params* grads,
                               void* scratch, hipStream_t s) {
    if (!feats || !ws || !scratch || !prob || !thresh || !params_ok(params, false) || !params_ok(grads, false) || vtd_dbhead_ws_bytes(n, H, W, 1) < 0)
        return -2802;
    if (((uintptr_t)feats & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255)) return -2803;
    const FwdLayout L = fwd_layout(n, H, W);
    const BwdLayout B = bwd_layout(n, H, W);
    const char* w = (const char*)ws;
    char* x = (char*)scratch;
    const float* y1 = (const float*)(w + L.y1);
    const half_t *a1 = (const half_t*)(w + L.a1), *z = (const half_t*)(w + L.z);
    const half_t* wt1d = (const half_t*)(w + L.wt1d);
    const float *zero = (const float*)(w + L.zero), *stat = (const float*)(w + L.stat);
    half_t *dz = (half_t*)(x + B.dz), *dy1 = (half_t*)(x + B.dy1);
    float *da1 = (float*)(x + B.da1), *coef2 = (float*)(x + B.coef2), *coef1 = (float*)(x + B.coef1), *slab = (float*)(x + B.slab);
    double *part = (double*)(x + B.part), *bpart = (double*)(x + B.bpart);
    Branches P, Gr;
    P.b[0] = params->branch[0]; P.b[1] = params->branch[1];
    Gr.b[0] = grads->branch[0]; Gr.b[1] = grads->branch[1];
    const int64_t M1 = (int64_t)n * H * W, M2 = 4 * M1;
    const int G1 = red_blocks(M1), G2 = red_blocks(M2);
    int rc;

    // ---- BN2 / ConvT2 level
    BwdArgs A2;
    std::memset(&A2, 0, sizeof(A2));
    A2.vh = z; A2.zshift = stat + 512; A2.stat = stat + 256; A2.s0 = prob; A2.s1 = thresh; A2.g0 = gprob; A2.g1 = gthresh;
    A2.n = n; A2.H2 = 2 * H; A2.W2 = 2 * W; A2.rows = M2; A2.per = rows_per_block(M2, G2);
    hipLaunchKernelGGL(dbhead_train_bwd_reduce_kernel<2>, dim3(G2), dim3(DHT_THREADS), 0, s, A2, P, part, bpart);
    hipLaunchKernelGGL(dbhead_train_bwd_finish_kernel<2>, dim3(1), dim3(128), 0, s, (const double*)part, (const double*)bpart, G2, M2, training, P, Gr,
                       A2.stat, coef2);
    hipLaunchKernelGGL(dbhead_train_bwd_form_kernel<2>, dim3(G2), dim3(DHT_THREADS), 0, s, A2, P, (const float*)coef2, dz, bpart);
    hipLaunchKernelGGL(dbhead_train_bias_finish_kernel, dim3(1), dim3(128), 0, s, (const double*)bpart, G2, Gr, 1);
    VTD_HIP_CHECK(hipGetLastError());

    // ---- ConvT1: input gradient (scaled by the BN2 pass's scale) and weight gradient
    for (int b = 0; b < 2; ++b) {
        ConvParams c = base_conv();
        c.in = dz + b * 64; c.wgt = wt1d + (int64_t)b * 64 * 256; c.bias = zero; c.out = da1 + b * 64; c.ldc = 128;
        c.cin_steps = 1; c.kw = 2; c.s_step = 128; c.r_step = 2 * W * 128; c.stride = 2;
        c.M = (int)M1; c.K = 256; c.cout = 64; c.cout_pad = 64; c.ho = H; c.wo = W;
        c.in_hp = 2 * H; c.in_wp = 2 * W; c.in_c = 128; c.in_y0 = 0; c.in_x0 = 0;
        c.flags = EPI_OUT_F32;
        if ((rc = vtd_launch_conv(c, -1, s))) return rc;
    }
    {
        WgArgs wa;
        wa.xc = 0;
        wa.a = a1; wa.lda = 256; wa.x = dz; wa.n = n; wa.H = H; wa.W = W; wa.rows = M1; wa.slab = slab;
        const int S = wgrad_slabs(M1, 1);
        wa.slab_len = slab_rows(M1, S);
        hipLaunchKernelGGL(dbhead_train_wgrad_kernel<1>, dim3(4 * S), dim3(DHT_THREADS), 0, s, wa);
        hipLaunchKernelGGL(dbhead_train_wgrad_reduce_kernel<1>, dim3(blocks_for(2 * 64 * 256)), dim3(DHT_THREADS), 0, s, (const float*)slab, S,
                           (const float*)(coef2 + 386), Gr);
        VTD_HIP_CHECK(hipGetLastError());
    }

    // ---- BN1 level
    BwdArgs A1;
    std::memset(&A1, 0, sizeof(A1));
    A1.vf = y1; A1.stat = stat; A1.da1 = da1; A1.inv_sc_in = coef2 + 386; A1.rows = M1; A1.per = rows_per_block(M1, G1);
    hipLaunchKernelGGL(dbhead_train_bwd_reduce_kernel<1>, dim3(G1), dim3(DHT_THREADS), 0, s, A1, P, part, bpart);
    hipLaunchKernelGGL(dbhead_train_bwd_finish_kernel<1>, dim3(1), dim3(128), 0, s, (const double*)part, (const double*)bpart, G1, M1, training, P, Gr,
                       A1.stat, coef1);
    hipLaunchKernelGGL(dbhead_train_bwd_form_kernel<1>, dim3(G1), dim3(DHT_THREADS), 0, s, A1, P, (const float*)coef1, dy1, bpart);
    hipLaunchKernelGGL(dbhead_train_bias_finish_kernel, dim3(1), dim3(128), 0, s, (const double*)bpart, G1, Gr, 0);
    VTD_HIP_CHECK(hipGetLastError());

    // ---- conv 3x3 weight gradient
    {
        WgArgs wa;
        wa.xc = 0;
        wa.a = dy1; wa.lda = 128; wa.x = (const half_t*)feats; wa.n = n; wa.H = H; wa.W = W; wa.rows = M1; wa.slab = slab;
        const int S = wgrad_slabs(M1, 0);
        wa.slab_len = slab_rows(M1, S);
        hipLaunchKernelGGL(dbhead_train_wgrad_kernel<0>, dim3(18 * S), dim3(DHT_THREADS), 0, s, wa);
        hipLaunchKernelGGL(dbhead_train_wgrad_reduce_kernel<0>, dim3(blocks_for(128 * 2304)), dim3(DHT_THREADS), 0, s, (const float*)slab, S,
                           (const float*)(coef1 + 386), Gr);
    }
    return -(int)hipGetLastError();
}

// dP2 after vtd_launch_dbhead_backward on the same scratch (sized by mode 2): reads dy1 and its two scales where the backward left them
int vtd_launch_dbhead_backward_input(int n, int H, int W, const vtd_dbhead_params* params, void* scratch, float* dfeats, float* dscale, hipStream_t s) {
    if (!scratch || !dfeats || !dscale || !params || vtd_dbhead_ws_bytes(n, H, W, 2) < 0) return -2802;
    for (int b = 0; b < 2; ++b)
        if (!params->branch[b].conv_w || ((uintptr_t)params->branch[b].conv_w & 3)) return -2802;
    if (((uintptr_t)scratch & 255) || ((uintptr_t)dfeats & 15) || ((uintptr_t)dscale & 7)) return -2803;
    const BwdLayout B = bwd_layout(n, H, W);
    const DgradLayout D = dgrad_layout(n, H, W);
    char* x = (char*)scratch;
    const half_t* dy1 = (const half_t*)(x + B.dy1);
    const float* coef1 = (const float*)(x + B.coef1);
    half_t *dy1p = (half_t*)(x + D.dy1p), *wd3 = (half_t*)(x + D.wd3);
    float* zero = (float*)(x + D.zero);
    Branches P;
    P.b[0] = params->branch[0]; P.b[1] = params->branch[1];
    const int64_t M1 = (int64_t)n * H * W;
    hipLaunchKernelGGL(dbhead_train_pack_dgrad_weights_kernel, dim3(blocks_for(PACK_DGRAD_ITEMS)), dim3(DHT_THREADS), 0, s, P, coef1, wd3, zero, dscale);
    hipLaunchKernelGGL(dbhead_train_pad_dy1_kernel, dim3(blocks_for((int64_t)n * (H + 2) * (W + 2) * 16)), dim3(DHT_THREADS), 0, s, dy1, n, H, W, dy1p);
    VTD_HIP_CHECK(hipGetLastError());
    ConvParams c = base_conv();
    c.in = dy1p; c.wgt = wd3; c.bias = zero; c.out = dfeats; c.ldc = 256; c.flags = EPI_OUT_F32;
    c.cin_steps = 2; c.kw = 3; c.s_step = 128; c.r_step = (W + 2) * 128;
    c.M = (int)M1; c.K = 1152; c.cout = 256; c.cout_pad = 256; c.ho = H; c.wo = W;
    c.in_hp = H + 2; c.in_wp = W + 2; c.in_c = 128; c.in_y0 = 0; c.in_x0 = 0;
    return vtd_launch_conv(c, -1, s);
}

int vtd_launch_dbhead_unpack_input_grad(const float* dfeats, const float* dscale, int n, int H, int W, float* out, hipStream_t s) {
    if (!dfeats || !dscale || !out || vtd_dbhead_ws_bytes(n, H, W, 2) < 0 || n > 65535) return -2802;
    if (((uintptr_t)dfeats & 15) || ((uintptr_t)dscale & 7) || ((uintptr_t)out & 3)) return -2803;
    const int HW = H * W;
    hipLaunchKernelGGL(dbhead_train_unpack_input_grad_kernel, dim3((HW + 63) / 64, 4, n), dim3(DHT_THREADS), 0, s, dfeats, dscale, HW, out);
    return -(int)hipGetLastError();
}
