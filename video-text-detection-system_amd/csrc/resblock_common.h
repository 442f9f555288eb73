// What the two ResNet BasicBlock training files share (resblock_train.hip: frozen-statistics BatchNorm; resblock_bn_train.hip: batch
// statistics): the padded-tap helpers, the ReLU mask, the identity add, the weight-gradient slab rules, the argument checks and the
// convolution descriptor.
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
