// What the ResNet block training files share (resblock_train.hip: BasicBlocks with frozen-statistics BatchNorm; resblock_bn_train.hip: batch
// statistics; bottleneck_train.hip: ResNet-50's Bottlenecks): the padded-tap helpers, the ReLU mask, the identity add, the weight-gradient
// slab rules, the argument checks and the convolution descriptor; and the kernels of the frozen-statistics path that take every width from
// their launch: the fold, the reduce's finish, the fp16 operand forming, the dgrad panel and the parameter gradients; and the 128-wide
// and 64-wide reduces, which ResNet-18's layer2 and ResNet-50's res3, and ResNet-18's layer1 and ResNet-50's res2, launch.
#ifndef VTD_RESBLOCK_COMMON_H
#define VTD_RESBLOCK_COMMON_H
#include "vtd_common.h"
#include "wgrad_mfma.h"
#include "../../include/vtd.h"

#include <cstring>

namespace {   // per translation unit, as every kernel of this library

constexpr int RB_THREADS = 256;
constexpr float RB_SCALE_TARGET = 16384.0f;

inline int64_t a256(int64_t x) { return (x + 255) & ~(int64_t)255; }
inline unsigned nblk(int64_t items) { return (unsigned)((items + RB_THREADS - 1) / RB_THREADS); }

inline int wg_slabs(int64_t rows) { int64_t s = (rows + 4095) / 4096; return (int)(s < 1 ? 1 : s > 8 ? 8 : s); }
inline int64_t slab_rows(int64_t rows, int s) { return ((rows + s - 1) / s + WG_KC - 1) / WG_KC * WG_KC; }
// W = 128 (one column tile): the slabs of a launch of `nqt` q-tiles.  Shape-only: 512 workgroups when the rows allow slabs of 1024
inline int wg_slabs128(int64_t rows, int nqt) {
    const int64_t want = (512 + nqt - 1) / nqt, can = (rows + 1023) / 1024;
    return (int)(want < can ? want : can < 1 ? 1 : can);
}
// the same rule with the column tiles counted (ResNet-50's res3, whose 512-wide gradients have four): workgroups = nqt x ctiles x slabs
inline int wg_slabs_tiles(int64_t rows, int nqt, int ctiles) { return wg_slabs128(rows, nqt * ctiles); }
inline int wg_nqt(int ksz, int xc) { return (ksz * ksz * xc + 127) / 128; }

// the one-pixel ring of a padded NHWC fp16 tensor of W channels.  One thread = 8 channels of one ring pixel.
__global__ __launch_bounds__(RB_THREADS) void rb_zero_ring_kernel(half_t* t, int n, int H, int Wd, int W) {
    const int Hp = H + 2, Wp = Wd + 2, R = 2 * Wp + 2 * H, C8 = W >> 3;
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    if (i >= (int64_t)n * R * C8) return;
    const int c8 = (int)(i % C8);
    const int64_t q = i / C8;
    const int r = (int)(q % R), img = (int)(q / R);
    int yp, xp;
    if (r < Wp) { yp = 0; xp = r; }
    else if (r < 2 * Wp) { yp = Hp - 1; xp = r - Wp; }
    else { const int k = r - 2 * Wp; yp = 1 + (k >> 1); xp = (k & 1) ? Wp - 1 : 0; }
    const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    *(half8*)(t + (((int64_t)img * Hp + yp) * Wp + xp) * W + c8 * 8) = z;
}

// out[m][c] = v[m][c] where the padded activation at pixel m is positive, else 0.  One thread = 4 channels.
__global__ __launch_bounds__(RB_THREADS) void rb_mask_kernel(const float* v, const half_t* act, int64_t rows, int H, int Wd, int W, float* out) {
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    const int C4 = W >> 2;
    if (i >= rows * C4) return;
    const int cq = (int)(i % C4);
    const int64_t m = i / C4;
    const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    const half_t* a = act + (((int64_t)img * (H + 2) + y + 1) * (Wd + 2) + x + 1) * W + 4 * cq;
    const floatx4 f = *(const floatx4*)(v + i * 4);
    floatx4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)a[e] > 0.f ? f[e] : 0.f;
    *(floatx4*)(out + i * 4) = o;
}

// dx = conv1^T(g1) (at g1's total scale) + g2 (at the incoming scale) brought to that scale: both multipliers are powers of two
__global__ __launch_bounds__(RB_THREADS) void rb_add_identity_kernel(float* dx, const float* g2, int64_t items, const float* sc2, const float* sc1) {
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    if (i >= items) return;
    const float mul = sc2[2] * sc1[2];
    floatx4 a = *(floatx4*)(dx + i * 4);
    const floatx4 b = *(const floatx4*)(g2 + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += b[e] * mul;
    *(floatx4*)(dx + i * 4) = a;
}

__global__ void rb_copy_scale_kernel(const float* sc, float* out) {
    if (threadIdx.x < 2) out[threadIdx.x] = sc[threadIdx.x];
}

// ---- kernels that take every width and extent from their launch: shared with bottleneck_train.hip -------------------------------------
// wp [W][ksz^2 cin], k = tap * cin + ci: half(w[co][ci][tap] gamma rstd); bias[co] = beta - mean gamma rstd
__global__ __launch_bounds__(RB_THREADS) void rb_fold_kernel(const float* w, const float* gam, const float* bet, const float* mean, const float* var,
                                                             float eps, int W, int cin, int taps, half_t* wp, float* bias) {
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    const int K = taps * cin;
    if (i < (int64_t)W * K) {
        const int co = (int)(i / K), k = (int)(i - (int64_t)co * K), tap = k / cin, ci = k - tap * cin;
        const float sc = gam[co] / sqrtf(var[co] + eps);
        wp[i] = (half_t)(w[((int64_t)co * cin + ci) * taps + tap] * sc);
    } else if (i < (int64_t)W * K + W) {
        const int co = (int)(i - (int64_t)W * K);
        bias[co] = bet[co] - mean[co] * (gam[co] / sqrtf(var[co] + eps));
    }
}

// v [rows][W] fp32, W = 256 or 512: thread t owns channel t (and t + 256 of a 512-wide v) over the rows of its workgroup, in row order:
// part[g][W] fp64, pmax[g]
__global__ __launch_bounds__(RB_THREADS) void rb_reduce_kernel(const float* v, int64_t rows, int64_t per, int W, double* part, float* pmax) {
    const int t = threadIdx.x;
    const bool two = W > 256;
    const int64_t m0 = (int64_t)blockIdx.x * per, m1 = m0 + per < rows ? m0 + per : rows;
    double s0 = 0.0, s1 = 0.0;
    float mx = 0.f;
    for (int64_t m = m0; m < m1; ++m) {
        const float a = v[m * W + t], b = two ? v[m * W + 256 + t] : 0.f;
        s0 += (double)a; s1 += (double)b;
        const float fa = fabsf(a), fb = fabsf(b);
        mx = fa > mx || fa != fa ? fa : mx;
        mx = fb > mx || fb != fb ? fb : mx;
    }
    part[(int64_t)blockIdx.x * W + t] = s0;
    if (two) part[(int64_t)blockIdx.x * W + 256 + t] = s1;
    __shared__ float shm[RB_THREADS];
    shm[t] = mx;
    __syncthreads();
    if (t == 0) {
        float m = shm[0];
        for (int k = 1; k < RB_THREADS; ++k) m = shm[k] > m || shm[k] != shm[k] ? shm[k] : m;
        pmax[blockIdx.x] = m;
    }
}

// v [rows][128] fp32: thread t owns channel t % 128 over one half of the workgroup's rows m0 .. m1 in row order, t < 128 the first
// ceil((m1 - m0) / 2) rows and t >= 128 the rest; part[g][c] = the first half's sum + the second half's, fp64; pmax[g]
__global__ __launch_bounds__(RB_THREADS) void rb_reduce128_kernel(const float* v, int64_t rows, int64_t per, double* part, float* pmax) {
    const int t = threadIdx.x, c = t & 127, hf = t >> 7;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t mid = m0 + (m1 - m0 + 1) / 2, lo = hf ? mid : m0, hi = hf ? m1 : mid;
    double s = 0.0;
    float mx = 0.f;
    for (int64_t m = lo; m < hi; ++m) {
        const float a = v[m * 128 + c], fa = fabsf(a);
        s += (double)a;
        mx = fa > mx || fa != fa ? fa : mx;
    }
    __shared__ double shs[128];
    __shared__ float shm[RB_THREADS];
    if (hf) shs[c] = s;
    shm[t] = mx;
    __syncthreads();
    if (!hf) part[(int64_t)blockIdx.x * 128 + c] = s + shs[c];
    if (t == 0) {
        float m = shm[0];
        for (int k = 1; k < RB_THREADS; ++k) m = shm[k] > m || shm[k] != shm[k] ? shm[k] : m;
        pmax[blockIdx.x] = m;
    }
}

// v [rows][64] fp32: thread t owns channel t % 64 over one quarter of the workgroup's rows m0 .. m1 in row order: quarter k = t / 64 takes
// rows m0 + ceil(k r / 4) .. m0 + ceil((k + 1) r / 4) - 1 of the r = m1 - m0; part[g][c] = (q0 + q1) + (q2 + q3), fp64; pmax[g]
__global__ __launch_bounds__(RB_THREADS) void rb_reduce64_kernel(const float* v, int64_t rows, int64_t per, double* part, float* pmax) {
    const int t = threadIdx.x, c = t & 63, k = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t r = m1 - m0, lo = m0 + (k * r + 3) / 4, hi = m0 + ((k + 1) * r + 3) / 4;
    double s = 0.0;
    float mx = 0.f;
    for (int64_t m = lo; m < hi; ++m) {
        const float a = v[m * 64 + c], fa = fabsf(a);
        s += (double)a;
        mx = fa > mx || fa != fa ? fa : mx;
    }
    __shared__ double shs[RB_THREADS];
    __shared__ float shm[RB_THREADS];
    shs[t] = s;
    shm[t] = mx;
    __syncthreads();
    if (k == 0) part[(int64_t)blockIdx.x * 64 + c] = (shs[c] + shs[64 + c]) + (shs[128 + c] + shs[192 + c]);
    if (t == 0) {
        float m = shm[0];
        for (int j = 1; j < RB_THREADS; ++j) m = shm[j] > m || shm[j] != shm[j] ? shm[j] : m;
        pmax[blockIdx.x] = m;
    }
}

// partials in workgroup order: sum[c] = the channel sum with the incoming scale undone (fp64); out_sc = {total scale, 1 / total,
// this stage's multiplier, 0}, the multiplier a power of two from max |v| (1 when that is zero or not finite)
__global__ __launch_bounds__(RB_THREADS) void rb_finish_kernel(const double* part, const float* pmax, int G, int W, const float* in_sc, double* sum,
                                                               float* out_sc) {
    const int t = threadIdx.x;
    for (int c = t; c < W; c += RB_THREADS) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += part[(int64_t)g * W + c];
        sum[c] = s * (double)in_sc[1];
    }
    if (t == 0) {
        float mx = pmax[0];
        for (int g = 1; g < G; ++g) mx = pmax[g] > mx || pmax[g] != pmax[g] ? pmax[g] : mx;
        const double tin = (double)in_sc[0];
        int e = 0;
        if (mx > 0.f && isfinite(mx)) e = (int)floor(log2((double)RB_SCALE_TARGET / (double)mx));
        const int ein = (tin > 0.0 && isfinite(tin)) ? ilogb(tin) : 0;
        int et = ein + e;
        et = et < -120 ? -120 : et > 120 ? 120 : et;
        e = et - ein;
        const double tot = tin * ldexp(1.0, e);
        out_sc[0] = (float)tot; out_sc[1] = (float)(1.0 / tot); out_sc[2] = ldexpf(1.0f, e); out_sc[3] = 0.f;
    }
}

// v times the multiplier as fp16: flat [rows][W] (when given) and a ring-padded plane [n][dil H + 2][dil Wd + 2][W] at pixel (dil y, dil x):
// dil = 1 fills the interior, dil = 2 the even positions of the stride-2 dgrad's zero-inserted plane.  One thread = 8 channels.
__global__ __launch_bounds__(RB_THREADS) void rb_form_kernel(const float* v, int64_t rows, const float* sc, int H, int Wd, int W, int dil, half_t* flat,
                                                             half_t* padded) {
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    const int C8 = W >> 3;
    if (i >= rows * C8) return;
    const float mul = sc[2];
    const floatx4 v0 = *(const floatx4*)(v + i * 8), v1 = *(const floatx4*)(v + i * 8 + 4);
    half8 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) { h[e] = (half_t)(v0[e] * mul); h[4 + e] = (half_t)(v1[e] * mul); }
    if (flat) *(half8*)(flat + i * 8) = h;
    const int64_t m = i / C8;
    const int c8 = (int)(i % C8), HW = H * Wd;
    const int img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    *(half8*)(padded + (((int64_t)img * (dil * H + 2) + dil * y + 1) * (dil * Wd + 2) + dil * x + 1) * W + c8 * 8) = h;
}

// wt [cin][taps * W]: row ci, k = tap' * W + co holds half(w[co][ci][taps - 1 - tap'] gamma rstd) (the window rotated by 180 degrees, the
// folded weights transposed, rounded as the forward packs them); a zero bias row of W entries
__global__ __launch_bounds__(RB_THREADS) void rb_pack_dgrad_kernel(const float* w, const float* gam, const float* var, float eps, int W, int cin, int taps,
                                                                   half_t* wt, float* zero) {
    const int i = blockIdx.x * RB_THREADS + threadIdx.x;
    const int K = taps * W;
    if (i < cin * K) {
        const int ci = i / K, k = i - ci * K, tap = k / W, co = k - tap * W;
        wt[i] = (half_t)(w[((int64_t)co * cin + ci) * taps + (taps - 1 - tap)] * (gam[co] / sqrtf(var[co] + eps)));
    } else if (i < cin * K + W) {
        zero[i - cin * K] = 0.f;
    }
}

// One workgroup per output channel c.  G[c][k] = the slabs summed in slab order (fp64) with the scale undone, k = tap * cin + ci;
// dW[c][ci][tap] = gamma rstd G; dbeta = s; dgamma = rstd (sum_k w[c][k] G[c][k] - mean s), the sum in fp64 in a fixed tree order
__global__ __launch_bounds__(RB_THREADS) void rb_param_kernel(const float* slab, int S, int cin, int taps, const float* sc, const double* sum, const float* w,
                                                              const float* gam, const float* mean, const float* var, float eps, float* dw, float* dgam,
                                                              float* dbet) {
    const int c = blockIdx.x, t = threadIdx.x, K = taps * cin;
    const double rstd = 1.0 / sqrt((double)var[c] + (double)eps), inv = (double)sc[1], f = (double)gam[c] * rstd;
    const int64_t nel = (int64_t)gridDim.x * K;
    double dot = 0.0;
    for (int k = t; k < K; k += RB_THREADS) {
        double G = 0.0;
        for (int s = 0; s < S; ++s) G += (double)slab[(int64_t)s * nel + (int64_t)c * K + k];
        G *= inv;
        const int tap = k / cin, ci = k - tap * cin;
        const int64_t wi = ((int64_t)c * cin + ci) * taps + tap;
        dw[wi] = (float)(f * G);
        dot += (double)w[wi] * G;
    }
    __shared__ double sh[RB_THREADS];
    sh[t] = dot;
    __syncthreads();
    for (int o = RB_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) {
        dgam[c] = (float)(rstd * (sh[0] - (double)mean[c] * sum[c]));
        dbet[c] = (float)sum[c];
    }
}

bool bn_ok(const float* w, const float* b, const float* m, const float* v) {
    return w && b && m && v && !(((uintptr_t)w | (uintptr_t)b | (uintptr_t)m | (uintptr_t)v) & 3);
}

bool params_ok(const vtd_basicblock_params* p, bool ds) {
    if (!p || !p->conv1_w || !p->conv2_w || (((uintptr_t)p->conv1_w | (uintptr_t)p->conv2_w) & 3)) return false;
    if (!bn_ok(p->bn1_w, p->bn1_b, p->bn1_mean, p->bn1_var) || !bn_ok(p->bn2_w, p->bn2_b, p->bn2_mean, p->bn2_var)) return false;
    if (ds && (!p->ds_w || ((uintptr_t)p->ds_w & 3) || !bn_ok(p->ds_bn_w, p->ds_bn_b, p->ds_bn_mean, p->ds_bn_var))) return false;
    return true;
}

bool grads_ok(const vtd_basicblock_params* p, bool ds) {
    if (!p || !p->conv1_w || !p->conv2_w || !p->bn1_w || !p->bn1_b || !p->bn2_w || !p->bn2_b) return false;
    if (ds && (!p->ds_w || !p->ds_bn_w || !p->ds_bn_b)) return false;
    return true;
}

ConvParams base_conv() {
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.k_hi_step = 32;
    p.stride = 1;
    return p;
}

// a 3x3 (pad 1) or 1x1 (pad 0) convolution at `stride` of a padded tap of hin x win pixels and cin channels into n x ho x wo rows of
// `cout` columns
ConvParams conv_of(int n, int ho, int wo, int cout, const half_t* in, int cin, int hin, int win, int ksz, int stride, const half_t* wgt,
                   const float* bias) {
    ConvParams c = base_conv();
    c.in = in; c.wgt = wgt; c.bias = bias;
    c.cin_steps = cin / 64; c.kw = ksz; c.s_step = cin; c.r_step = (win + 2) * cin;
    c.M = n * ho * wo; c.K = ksz * ksz * cin; c.cout = cout; c.cout_pad = cout; c.ho = ho; c.wo = wo;
    c.in_hp = hin + 2; c.in_wp = win + 2; c.in_c = cin; c.in_y0 = c.in_x0 = ksz == 3 ? 0 : 1; c.stride = stride;
    return c;
}

}  // namespace

#endif  // VTD_RESBLOCK_COMMON_H
