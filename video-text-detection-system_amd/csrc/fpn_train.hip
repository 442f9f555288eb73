// FPN training (text_detector.py:31-56 FeaturePyramidNetwork, the wiring SURVEY.md B.3 / build_detector_graph implement), forward and
// backward, over a frozen trunk: the caller hands in the four trunk taps C2..C5 as ring-padded NHWC fp16 tensors (ring 1) and gets P2 in
// the layout the DB-head training kernels read.  Level lv = 0..3 is C2..C5 (H_lv = h5 << (3 - lv), C_lv = c5_channels >> (3 - lv)) and
// belongs to fpn.inner_blocks[3 - lv].  There is no nonlinearity and no BatchNorm: the backward is linear in dP2.
//
// Forward:
//   pack_weights     torch's fp32 parameters -> fp16 GEMM panels and fp32 bias rows, on the device, every call
//   zero_ring        the one-pixel rings of padded L2 and of the padded P2 output
//   conv 1x1 x 4     L5 = inner[0](C5); L(k) = inner[5-k](C(k)) + up2(L(k+1)): conv_igemm.hip with EPI_RESIDUAL, res_shift = 1 -> padded fp16
//   conv 3x3         P2 = layer_blocks[3](L2), K = 2304, N = 256 (conv_igemm.hip) -> padded fp16; padded L2 stays in the workspace
// Backward, dP2 as vtd_dbhead_train_backward_input leaves it (NHWC fp32 times dscale[0], a power of two):
//   reduce / finish  per-channel fp64 sums (= the bias gradient) and max |.| of a gradient tensor; a power-of-two scale from the maximum
//   form             the tensor times that scale as fp16: flat [M][256] (the weight gradient's A operand) and, for dP2, ring-padded too
//   wgrad<0>         dW_layer3[256][2304] = sum_m dP2[m]^T im2col(L2)[m] (wgrad_mfma.h, two 128-column tiles), slabs summed in order
//   conv 3x3         dL2 = conv3x3^T(dP2): window rotated by 180 degrees, weights transposed, K = 2304 (conv_igemm.hip) -> fp32, scaled
//   per level        dL(k+1) = sumpool2x2(dL(k)) in fp32 (the adjoint of the nearest up-sampling); reduce / finish / form; wgrad<2>
//                    dW_inner[256][C_k] = sum_m dL(k)[m]^T C(k)[m]
// Input gradients (on request, after the backward, from the dL(k) and scales it left in the scratch):
//   per level        pack inner_w[5-k]^T as an fp16 panel [C_k][256]; form dL(k) times its scale as fp16 again (the bits the weight gradient
//                    read); dC(k) = dL(k) inner_w[5-k]: one GEMM, M = n h w, K = 256, N = C_k (conv_igemm.hip as a 1x1 convolution over
//                    the flat operand) -> NHWC fp32 at dL(k)'s total scale
// Every reduction has a grid that depends on the shape only and a fixed summation order, and no atomics: bitwise repeatable.
#include "vtd_common.h"
#include "wgrad_mfma.h"
#include "../../include/vtd.h"

#include <cstring>

#include "conv_kernels.h"

namespace {

constexpr int FT_THREADS = 256;
constexpr int FT_MAX_RED_BLOCKS = 1024;
constexpr float FT_SCALE_TARGET = 16384.0f;  // scaled operands stay below 2^14 (fp16 max 65504)

__host__ __device__ inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
inline unsigned blocks_for(int64_t items) { return (unsigned)((items + FT_THREADS - 1) / FT_THREADS); }

inline int red_blocks(int64_t rows) {
    int64_t g = (rows + 511) / 512;
    return (int)(g < 1 ? 1 : g > FT_MAX_RED_BLOCKS ? FT_MAX_RED_BLOCKS : g);
}
inline int64_t rows_per_block(int64_t rows, int g) { return (rows + g - 1) / g; }
// weight-gradient slabs (split over M): 3x3 as the head's conv, 1x1 as its ConvT1
inline int wgrad_slabs(int64_t rows, bool k3) {
    const int64_t per = k3 ? 8192 : 4096, cap = k3 ? 64 : 256;
    int64_t s = (rows + per - 1) / per;
    return (int)(s < 1 ? 1 : s > cap ? cap : s);
}
inline int64_t slab_rows(int64_t rows, int s) { return (rows_per_block(rows, s) + WG_KC - 1) / WG_KC * WG_KC; }

// ---- geometry: given by the C5 size; every level below is exactly twice the one above
struct Geo {
    int n, h[4], w[4], c[4];
    int64_t m[4];   // n h w
};

bool make_geo(int n, int h5, int w5, int c5, Geo& g) {
    if (n <= 0 || h5 <= 0 || w5 <= 0 || n > (1 << 20) || h5 > (1 << 12) || w5 > (1 << 12)) return false;
    if (c5 < 512 || c5 > 4096 || (c5 & 511)) return false;   // C2 = c5 / 8 is a multiple of 64 (one K-step of the GEMMs)
    g.n = n;
    for (int lv = 0; lv < 4; ++lv) {
        g.h[lv] = h5 << (3 - lv); g.w[lv] = w5 << (3 - lv); g.c[lv] = c5 >> (3 - lv);
        g.m[lv] = (int64_t)n * g.h[lv] * g.w[lv];
    }
    if (g.m[0] * 4 >= (1ll << 31)) return false;
    const int64_t cmax = g.c[0] > 256 ? g.c[0] : 256;
    if ((int64_t)n * (g.h[0] + 2) * (g.w[0] + 2) * cmax >= (1ll << 31)) return false;   // element offsets of the padded tensors fit an int
    for (int lv = 1; lv < 4; ++lv)
        if ((int64_t)n * (g.h[lv] + 2) * (g.w[lv] + 2) * g.c[lv] >= (1ll << 31)) return false;
    return true;
}

// ---- workspace layout (one function for the size query and every call) ----------------------------------------------------------------
struct FwdLayout {
    int64_t L[4], wi[4], w3, bias, total;
};
struct BwdLayout {
    int64_t ah, dp2p, dl[4], wd3, zero, part, pmax, sc, slab, total;
};

FwdLayout fwd_layout(const Geo& g) {
    FwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t r = o; o += align256(bytes); return r; };
    for (int lv = 0; lv < 4; ++lv) L.L[lv] = take((int64_t)g.n * (g.h[lv] + 2) * (g.w[lv] + 2) * 256 * 2);
    for (int lv = 0; lv < 4; ++lv) L.wi[lv] = take((int64_t)256 * g.c[lv] * 2);
    L.w3 = take((int64_t)256 * 2304 * 2);
    L.bias = take(5 * 256 * 4);   // inner[3 - lv] at row lv, layer_blocks[3] at row 4
    L.total = o;
    return L;
}

BwdLayout bwd_layout(const Geo& g) {
    BwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t r = o; o += align256(bytes); return r; };
    L.ah = take(g.m[0] * 256 * 2);
    L.dp2p = take((int64_t)g.n * (g.h[0] + 2) * (g.w[0] + 2) * 256 * 2);
    for (int lv = 0; lv < 4; ++lv) L.dl[lv] = take(g.m[lv] * 256 * 4);
    L.wd3 = take((int64_t)256 * 2304 * 2);
    L.zero = take(256 * 4);
    L.part = take((int64_t)FT_MAX_RED_BLOCKS * 256 * 8);
    L.pmax = take((int64_t)FT_MAX_RED_BLOCKS * 4);
    L.sc = take(5 * 4 * 4);   // per stage (dP2, then the four levels): {total scale, 1 / total, this stage's multiplier, unused}
    int64_t slab = (int64_t)wgrad_slabs(g.m[0], true) * 256 * 2304 * 4;
    for (int lv = 0; lv < 4; ++lv) {
        const int64_t s = (int64_t)wgrad_slabs(g.m[lv], false) * 256 * g.c[lv] * 4;
        slab = s > slab ? s : slab;
    }
    L.slab = take(slab);
    L.total = o;
    return L;
}

// the input-gradient call's buffers lie behind the backward's scratch, which keeps its own layout: the backward writes the same bits into
// a scratch of either size
struct InLayout {
    int64_t wt[4], zero, total;
};

InLayout in_layout(const Geo& g) {
    InLayout L;
    int64_t o = bwd_layout(g).total;
    auto take = [&](int64_t bytes) { const int64_t r = o; o += align256(bytes); return r; };
    for (int lv = 0; lv < 4; ++lv) L.wt[lv] = take((int64_t)g.c[lv] * 256 * 2);
    L.zero = take((int64_t)g.c[3] * 4);
    L.total = o;
    return L;
}

// ---- layout kernels ---------------------------------------------------------------------------------------------------------------

// NCHW [n][C][H][W] (fp32 or fp16) -> padded NHWC fp16, ring zeroed.  One thread = 8 channels of one padded pixel.
template <typename T>
__global__ __launch_bounds__(FT_THREADS) void fpn_train_pack_tap_kernel(const T* x, int n, int Cc, int H, int W, half_t* out) {
    const int Hp = H + 2, Wp = W + 2, C8 = Cc >> 3;
    const int64_t total = (int64_t)n * Hp * Wp * C8;
    const int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    if (i >= total) return;
    const int xp = (int)(i % Wp);
    const int64_t r = i / Wp;
    const int c8 = (int)(r % C8);
    const int64_t r2 = r / C8;
    const int yp = (int)(r2 % Hp), img = (int)(r2 / Hp);
    half8 v;
    const int y = yp - 1, xx = xp - 1;
    const bool inside = y >= 0 && y < H && xx >= 0 && xx < W;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = inside ? (half_t)(float)x[(((int64_t)img * Cc + c8 * 8 + e) * H + y) * W + xx] : (half_t)0.f;
    *(half8*)(out + (((int64_t)img * Hp + yp) * Wp + xp) * Cc + c8 * 8) = v;
}

// the one-pixel ring of a padded NHWC fp16 tensor of 256 channels.  One thread = 8 channels of one ring pixel.
__global__ __launch_bounds__(FT_THREADS) void fpn_train_zero_ring_kernel(half_t* t, int n, int H, int W) {
    const int Hp = H + 2, Wp = W + 2, R = 2 * Wp + 2 * H;
    const int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    if (i >= (int64_t)n * R * 32) return;
    const int c8 = (int)(i & 31);
    const int64_t q = i >> 5;
    const int r = (int)(q % R), img = (int)(q / R);
    int yp, xp;
    if (r < Wp) { yp = 0; xp = r; }
    else if (r < 2 * Wp) { yp = Hp - 1; xp = r - Wp; }
    else { const int k = r - 2 * Wp; yp = 1 + (k >> 1); xp = (k & 1) ? Wp - 1 : 0; }
    const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    *(half8*)(t + (((int64_t)img * Hp + yp) * Wp + xp) * 256 + c8 * 8) = z;
}

// padded NHWC fp16 [n][H+2][W+2][256] -> NCHW fp32 [n][256][H][W].  Workgroup = 64 pixels of one image x 64 channels through an LDS tile.
__global__ __launch_bounds__(FT_THREADS) void fpn_train_unpack_p2_kernel(const half_t* p2, int H, int W, float* out) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x, lane = t & 63, row = t >> 6, HW = H * W;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, img = blockIdx.z;
    for (int r = row; r < 64; r += 4) {
        const int p = p0 + r, y = p / W, x = p - y * W;
        tile[r][lane] = p < HW ? (float)p2[(((int64_t)img * (H + 2) + y + 1) * (W + 2) + x + 1) * 256 + c0 + lane] : 0.f;
    }
    __syncthreads();
    for (int r = row; r < 64; r += 4) {
        const int p = p0 + lane;
        if (p < HW) out[((int64_t)img * 256 + c0 + r) * HW + p] = tile[lane][r];
    }
}

// NCHW fp32 [n][256][H][W] -> NHWC fp32 [n][H][W][256]: the mirror of dbhead_train_unpack_input_grad_kernel (an upstream gradient of P2
// handed to the stand-alone module, with dscale = {1, 1})
__global__ __launch_bounds__(FT_THREADS) void fpn_train_pack_grad_kernel(const float* g, int HW, float* out) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x, lane = t & 63, row = t >> 6;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, img = blockIdx.z;
    for (int r = row; r < 64; r += 4) {
        const int p = p0 + lane;
        tile[r][lane] = p < HW ? g[((int64_t)img * 256 + c0 + r) * HW + p] : 0.f;
    }
    __syncthreads();
    for (int r = row; r < 64; r += 4) {
        const int p = p0 + r;
        if (p < HW) out[((int64_t)img * HW + p) * 256 + c0 + lane] = tile[lane][r];
    }
}

// ---- weight packing ---------------------------------------------------------------------------------------------------------------
struct Params {
    const float* iw[4];   // by level: iw[lv] = fpn.inner_blocks[3 - lv].weight [256][C_lv]
    const float* ib[4];
    const float* lw;      // fpn.layer_blocks[3].weight [256][256][3][3]
    const float* lb;
};
struct WsPanels {
    half_t* wi[4];
    half_t* w3;
    float* bias;
};

// wi[lv] [256][C_lv] (K = ci contiguous: torch's own order), w3 [256][2304] row co, k = (ky*3+kx)*256 + ci, bias rows [5][256]
__global__ __launch_bounds__(FT_THREADS) void fpn_train_pack_weights_kernel(Params P, WsPanels O, int c2) {
    int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    for (int lv = 0; lv < 4; ++lv) {
        const int64_t nel = (int64_t)256 * (c2 << lv);
        if (i < nel) { O.wi[lv][i] = (half_t)P.iw[lv][i]; return; }
        i -= nel;
    }
    if (i < 256 * 2304) {
        const int co = (int)i / 2304, k = (int)i % 2304, tap = k / 256, ci = k % 256;
        O.w3[i] = (half_t)P.lw[(co * 256 + ci) * 9 + tap];
        return;
    }
    i -= 256 * 2304;
    if (i < 5 * 256) O.bias[i] = i < 4 * 256 ? P.ib[i >> 8][i & 255] : P.lb[i & 255];
}

// wd3 [256][2304]: row ci, k = tap' * 256 + co holds w[co][ci][8 - tap'] (the window rotated by 180 degrees), rounded to fp16 as the
// forward packs it; a zero bias row
__global__ __launch_bounds__(FT_THREADS) void fpn_train_pack_dgrad_weights_kernel(const float* lw, half_t* wd3, float* zero) {
    const int i = blockIdx.x * FT_THREADS + threadIdx.x;
    if (i < 256 * 2304) {
        const int ci = i / 2304, k = i % 2304, tap = k / 256, co = k % 256;
        wd3[i] = (half_t)lw[(co * 256 + ci) * 9 + (8 - tap)];
    } else if (i < 256 * 2304 + 256) {
        zero[i - 256 * 2304] = 0.f;
    }
}

// wt [C][256]: row ci, k = co holds w[co][ci] (the lateral's weights transposed), rounded to fp16 as the forward packs it; a zero bias
// row of C floats
__global__ __launch_bounds__(FT_THREADS) void fpn_train_pack_input_weights_kernel(const float* w, int Cc, half_t* wt, float* zero) {
    const int i = blockIdx.x * FT_THREADS + threadIdx.x;
    if (i < 256 * Cc) {
        const int ci = i >> 8, co = i & 255;
        wt[i] = (half_t)w[co * Cc + ci];
    } else if (i < 256 * Cc + Cc) {
        zero[i - 256 * Cc] = 0.f;
    }
}

// out[lv] = {total scale, 1 / total} of the requested levels, from the backward's per-stage scales
__global__ void fpn_train_copy_scales_kernel(const float* sc, int mask, float* out) {
    const int t = threadIdx.x, lv = t >> 1;
    if (t < 8 && ((mask >> lv) & 1)) out[t] = sc[4 * (lv + 1) + (t & 1)];
}

// NHWC fp32 [n][HW][C] times sc[0] -> NCHW fp32 [n][C][HW], the scale undone (sc[1] = 1 / scale, exact: a power of two).  Workgroup =
// 64 pixels of one image x 64 channels through an LDS tile.
__global__ __launch_bounds__(FT_THREADS) void fpn_train_unpack_tap_grad_kernel(const float* g, const float* sc, int Cc, int HW, float* out) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x, lane = t & 63, row = t >> 6;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, img = blockIdx.z;
    const float inv = sc[1];
    for (int r = row; r < 64; r += 4) {
        const int p = p0 + r;
        tile[r][lane] = p < HW ? g[((int64_t)img * HW + p) * Cc + c0 + lane] * inv : 0.f;
    }
    __syncthreads();
    for (int r = row; r < 64; r += 4) {
        const int p = p0 + lane;
        if (p < HW) out[((int64_t)img * Cc + c0 + r) * HW + p] = tile[lane][r];
    }
}

// ---- backward: sums, scales, operands -------------------------------------------------------------------------------------------------
// v [rows][256] fp32.  Thread (channel quad cq = t % 64, row lane r = t / 64): fp64 sums over the rows of one workgroup, the four row
// lanes added in order: part[g][256]; pmax[g] = max |v| of the workgroup.
__global__ __launch_bounds__(FT_THREADS) void fpn_train_reduce_kernel(const float* v, int64_t rows, int64_t per, double* part, float* pmax) {
    const int t = threadIdx.x, cq = t & 63, r = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * per, m1 = m0 + per < rows ? m0 + per : rows;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    float mx = 0.f;
    for (int64_t m = m0 + r; m < m1; m += 4) {
        const floatx4 f = *(const floatx4*)(v + m * 256 + 4 * cq);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s[e] += (double)f[e];
            const float a = fabsf(f[e]);
            mx = a > mx || a != a ? a : mx;   // a NaN sticks: the stage is then not scaled
        }
    }
    __shared__ double sh[4][256];
    __shared__ float shm[FT_THREADS];
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[r][4 * cq + e] = s[e];
    shm[t] = mx;
    __syncthreads();
    part[(int64_t)blockIdx.x * 256 + t] = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
    if (t == 0) {
        float m = shm[0];
        for (int k = 1; k < FT_THREADS; ++k) m = shm[k] > m || shm[k] != shm[k] ? shm[k] : m;
        pmax[blockIdx.x] = m;
    }
}

// One workgroup, one thread per channel: partials in workgroup order; bias gradient = sum / (scale the tensor carries, in_sc[0]); this
// stage's power-of-two multiplier from max |v| (1 when that is zero or not finite); out_sc = {total scale, 1 / total, multiplier, 0}
__global__ __launch_bounds__(256) void fpn_train_finish_kernel(const double* part, const float* pmax, int G, const float* in_sc, float* bias_grad,
                                                               float* out_sc) {
    const int c = threadIdx.x;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(int64_t)g * 256 + c];
    bias_grad[c] = (float)(s * (double)in_sc[1]);
    if (c == 0) {
        float mx = pmax[0];
        for (int g = 1; g < G; ++g) mx = pmax[g] > mx || pmax[g] != pmax[g] ? pmax[g] : mx;
        const double tin = (double)in_sc[0];
        int e = 0;
        if (mx > 0.f && isfinite(mx)) e = (int)floor(log2((double)FT_SCALE_TARGET / (double)mx));
        const int ein = (tin > 0.0 && isfinite(tin)) ? ilogb(tin) : 0;
        int et = ein + e;
        et = et < -120 ? -120 : et > 120 ? 120 : et;   // the total scale and its inverse stay normal fp32 numbers
        e = et - ein;
        const double tot = tin * ldexp(1.0, e);
        out_sc[0] = (float)tot;
        out_sc[1] = (float)(1.0 / tot);
        out_sc[2] = ldexpf(1.0f, e);
        out_sc[3] = 0.f;
    }
}

// v * multiplier as fp16: flat [rows][256] and (padded != null) the interior of a ring-padded [n][H+2][W+2][256].  One thread = 8 channels.
__global__ __launch_bounds__(FT_THREADS) void fpn_train_form_kernel(const float* v, int64_t rows, const float* sc, int H, int W, half_t* flat,
                                                                    half_t* padded) {
    const int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    if (i >= rows * 32) return;
    const float mul = sc[2];
    const floatx4 v0 = *(const floatx4*)(v + i * 8), v1 = *(const floatx4*)(v + i * 8 + 4);
    half8 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) { h[e] = (half_t)(v0[e] * mul); h[4 + e] = (half_t)(v1[e] * mul); }
    *(half8*)(flat + i * 8) = h;
    if (padded) {
        const int64_t m = i >> 5;
        const int c8 = (int)(i & 31), HW = H * W;
        const int img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / W, x = rem - y * W;
        *(half8*)(padded + (((int64_t)img * (H + 2) + y + 1) * (W + 2) + x + 1) * 256 + c8 * 8) = h;
    }
}

// out [n][h][w][256] = the 2x2 sums of in [n][2h][2w][256], fp32: the adjoint of the nearest-neighbour up-sampling.  One thread = 4 channels.
__global__ __launch_bounds__(FT_THREADS) void fpn_train_sumpool_kernel(const float* in, int n, int h, int w, float* out) {
    const int64_t i = (int64_t)blockIdx.x * FT_THREADS + threadIdx.x;
    if (i >= (int64_t)n * h * w * 64) return;
    const int cq = (int)(i & 63);
    const int64_t m = i >> 6;
    const int x = (int)(m % w);
    const int64_t r = m / w;
    const int y = (int)(r % h), img = (int)(r / h);
    const float* src = in + (((int64_t)img * 2 * h + 2 * y) * 2 * w + 2 * x) * 256 + 4 * cq;
    const floatx4 a = *(const floatx4*)src, b = *(const floatx4*)(src + 256);
    const floatx4 c = *(const floatx4*)(src + (int64_t)2 * w * 256), d = *(const floatx4*)(src + (int64_t)2 * w * 256 + 256);
    floatx4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (a[e] + b[e]) + (c[e] + d[e]);
    *(floatx4*)(out + i * 4) = o;
}

// slabs summed in slab order, scale undone, written in torch's layout.  K3: slab [256][2304] (q = tap * 256 + ci) -> [co][ci][3][3];
// otherwise slab [256][C] is torch's [co][ci][1][1] already
template <bool K3>
__global__ __launch_bounds__(FT_THREADS) void fpn_train_wgrad_reduce_kernel(const float* slab, int S, int nel, const float* sc, float* out) {
    const int i = blockIdx.x * FT_THREADS + threadIdx.x;
    if (i >= nel) return;
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += (double)slab[(int64_t)k * nel + i];
    const float g = (float)(s * (double)sc[1]);
    if constexpr (K3) {
        const int p = i / 2304, q = i % 2304, tap = q / 256, ci = q % 256;
        out[(p * 256 + ci) * 9 + tap] = g;
    } else {
        out[i] = g;
    }
}

bool params_ok(const vtd_fpn_params* p) {
    if (!p) return false;
    for (int i = 0; i < 4; ++i)
        if (!p->inner_w[i] || !p->inner_b[i] || ((uintptr_t)p->inner_w[i] & 3) || ((uintptr_t)p->inner_b[i] & 3)) return false;
    return p->layer_w && p->layer_b && !((uintptr_t)p->layer_w & 3) && !((uintptr_t)p->layer_b & 3);
}

// 0, -2902 (a tap is missing) or -2903 (a tap is not 16-byte aligned)
int taps_ok(const void* const* taps) {
    if (!taps) return -2902;
    for (int lv = 0; lv < 4; ++lv)
        if (!taps[lv]) return -2902;
    for (int lv = 0; lv < 4; ++lv)
        if ((uintptr_t)taps[lv] & 15) return -2903;
    return 0;
}

ConvParams base_conv() {
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.k_hi_step = 32;
    p.stride = 1;
    return p;
}

}  // namespace

int64_t vtd_fpn_ws_bytes(int n, int h5, int w5, int c5, int mode) {
    Geo g;
    if (!make_geo(n, h5, w5, c5, g) || mode < 0 || mode > 1) return -2902;
    return mode ? bwd_layout(g).total : fwd_layout(g).total;
}

int64_t vtd_fpn_input_ws_bytes(int n, int h5, int w5, int c5) {
    Geo g;
    if (!make_geo(n, h5, w5, c5, g)) return -2902;
    return in_layout(g).total;
}

int vtd_launch_fpn_unpack_tap_grad(const float* g, const float* sc, int n, int channels, int H, int W, float* out, hipStream_t s) {
    if (!g || !sc || !out || n <= 0 || H <= 0 || W <= 0 || n > 65535 || channels < 64 || channels > 4096 || (channels & 63) ||
        (int64_t)n * H * W * 4 >= (1ll << 31) || (int64_t)H * W * channels >= (1ll << 31))
        return -2902;
    if (((uintptr_t)g & 15) || ((uintptr_t)sc & 7) || ((uintptr_t)out & 3)) return -2903;
    hipLaunchKernelGGL(fpn_train_unpack_tap_grad_kernel, dim3((H * W + 63) / 64, channels / 64, n), dim3(FT_THREADS), 0, s, g, sc, channels, H * W, out);
    return -(int)hipGetLastError();
}

int vtd_launch_fpn_pack_tap(const void* x, int dtype, int n, int channels, int H, int W, void* out, hipStream_t s) {
    if (!x || !out || n <= 0 || H <= 0 || W <= 0 || channels < 64 || channels > 4096 || (channels & 63) || (dtype != 0 && dtype != 1)) return -2902;
    if ((int64_t)n * (H + 2) * (W + 2) * channels >= (1ll << 31)) return -2902;
    if ((uintptr_t)out & 15) return -2903;
    const int64_t items = (int64_t)n * (H + 2) * (W + 2) * (channels >> 3);
    if (dtype == 0)
        hipLaunchKernelGGL(fpn_train_pack_tap_kernel<float>, dim3(blocks_for(items)), dim3(FT_THREADS), 0, s, (const float*)x, n, channels, H, W, (half_t*)out);
    else
        hipLaunchKernelGGL(fpn_train_pack_tap_kernel<half_t>, dim3(blocks_for(items)), dim3(FT_THREADS), 0, s, (const half_t*)x, n, channels, H, W, (half_t*)out);
    return -(int)hipGetLastError();
}

int vtd_launch_fpn_unpack_p2(const void* p2, int n, int H, int W, float* out, hipStream_t s) {
    if (!p2 || !out || n <= 0 || H <= 0 || W <= 0 || n > 65535 || (int64_t)n * (H + 2) * (W + 2) * 256 >= (1ll << 31)) return -2902;
    if (((uintptr_t)p2 & 15) || ((uintptr_t)out & 3)) return -2903;
    hipLaunchKernelGGL(fpn_train_unpack_p2_kernel, dim3((H * W + 63) / 64, 4, n), dim3(FT_THREADS), 0, s, (const half_t*)p2, H, W, out);
    return -(int)hipGetLastError();
}

int vtd_launch_fpn_pack_grad(const float* g, int n, int H, int W, float* out, hipStream_t s) {
    if (!g || !out || n <= 0 || H <= 0 || W <= 0 || n > 65535 || (int64_t)n * H * W * 4 >= (1ll << 31)) return -2902;
    if (((uintptr_t)g & 3) || ((uintptr_t)out & 15)) return -2903;
    hipLaunchKernelGGL(fpn_train_pack_grad_kernel, dim3((H * W + 63) / 64, 4, n), dim3(FT_THREADS), 0, s, g, H * W, out);
    return -(int)hipGetLastError();
}

int vtd_launch_fpn_forward(const void* const* taps, int n, int h5, int w5, int c5, const vtd_fpn_params* params, void* ws, void* p2_out, hipStream_t s) {
    Geo g;
    if (!ws || !p2_out || !params_ok(params) || !make_geo(n, h5, w5, c5, g)) return -2902;
    int rc = taps_ok(taps);
    if (rc) return rc;
    if (((uintptr_t)ws & 255) || ((uintptr_t)p2_out & 15)) return -2903;
    const FwdLayout L = fwd_layout(g);
    char* w = (char*)ws;
    Params P;
    WsPanels O;
    half_t* lat[4];
    for (int lv = 0; lv < 4; ++lv) {
        P.iw[lv] = params->inner_w[3 - lv]; P.ib[lv] = params->inner_b[3 - lv];
        O.wi[lv] = (half_t*)(w + L.wi[lv]);
        lat[lv] = (half_t*)(w + L.L[lv]);
    }
    P.lw = params->layer_w; P.lb = params->layer_b;
    O.w3 = (half_t*)(w + L.w3);
    O.bias = (float*)(w + L.bias);
    int64_t items = 256 * 2304 + 5 * 256;
    for (int lv = 0; lv < 4; ++lv) items += (int64_t)256 * g.c[lv];
    hipLaunchKernelGGL(fpn_train_pack_weights_kernel, dim3(blocks_for(items)), dim3(FT_THREADS), 0, s, P, O, g.c[0]);
    const int64_t ring = (int64_t)n * (2 * (g.w[0] + 2) + 2 * g.h[0]) * 32;
    hipLaunchKernelGGL(fpn_train_zero_ring_kernel, dim3(blocks_for(ring)), dim3(FT_THREADS), 0, s, lat[0], n, g.h[0], g.w[0]);
    hipLaunchKernelGGL(fpn_train_zero_ring_kernel, dim3(blocks_for(ring)), dim3(FT_THREADS), 0, s, (half_t*)p2_out, n, g.h[0], g.w[0]);
    VTD_HIP_CHECK(hipGetLastError());
    for (int lv = 3; lv >= 0; --lv) {   // laterals, coarsest first: L(lv) = inner(C(lv)) + up2(L(lv + 1))
        const int H = g.h[lv], W = g.w[lv], Cc = g.c[lv];
        ConvParams c = base_conv();
        c.in = (const half_t*)taps[lv]; c.wgt = O.wi[lv]; c.bias = O.bias + lv * 256; c.out = lat[lv];
        c.cin_steps = Cc / 64; c.kw = 1; c.s_step = Cc; c.r_step = (W + 2) * Cc;
        c.M = (int)g.m[lv]; c.K = Cc; c.cout = 256; c.cout_pad = 256; c.ho = H; c.wo = W;
        c.in_hp = H + 2; c.in_wp = W + 2; c.in_c = Cc; c.in_y0 = 1; c.in_x0 = 1;
        c.out_hp = H + 2; c.out_wp = W + 2; c.out_c = 256; c.out_ring = 1;
        if (lv < 3) {
            c.flags = EPI_RESIDUAL; c.res = lat[lv + 1];
            c.res_hp = g.h[lv + 1] + 2; c.res_wp = g.w[lv + 1] + 2; c.res_ring = 1; c.res_shift = 1;
        }
        if ((rc = vtd_launch_conv(c, -1, s))) return rc;
    }
    {   // P2 = conv 3x3 of padded L2
        const int H = g.h[0], W = g.w[0];
        ConvParams c = base_conv();
        c.in = lat[0]; c.wgt = O.w3; c.bias = O.bias + 4 * 256; c.out = p2_out;
        c.cin_steps = 4; c.kw = 3; c.s_step = 256; c.r_step = (W + 2) * 256;
        c.M = (int)g.m[0]; c.K = 2304; c.cout = 256; c.cout_pad = 256; c.ho = H; c.wo = W;
        c.in_hp = H + 2; c.in_wp = W + 2; c.in_c = 256; c.in_y0 = 0; c.in_x0 = 0;
        c.out_hp = H + 2; c.out_wp = W + 2; c.out_c = 256; c.out_ring = 1;
        return vtd_launch_conv(c, -1, s);
    }
}

int vtd_launch_fpn_backward(const void* const* taps, int n, int h5, int w5, int c5, const vtd_fpn_params* params, const void* ws, const float* dp2,
                            const float* dscale, const vtd_fpn_params* grads, void* scratch, hipStream_t s) {
    Geo g;
    if (!ws || !dp2 || !dscale || !scratch || !params || !params->layer_w || ((uintptr_t)params->layer_w & 3) || !params_ok(grads) ||
        !make_geo(n, h5, w5, c5, g))
        return -2902;
    int rc = taps_ok(taps);
    if (rc) return rc;
    if (((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255) || ((uintptr_t)dp2 & 15) || ((uintptr_t)dscale & 7)) return -2903;
    const FwdLayout L = fwd_layout(g);
    const BwdLayout B = bwd_layout(g);
    char* x = (char*)scratch;
    const half_t* l2 = (const half_t*)((const char*)ws + L.L[0]);
    half_t *ah = (half_t*)(x + B.ah), *dp2p = (half_t*)(x + B.dp2p), *wd3 = (half_t*)(x + B.wd3);
    float *zero = (float*)(x + B.zero), *pmax = (float*)(x + B.pmax), *sc = (float*)(x + B.sc), *slab = (float*)(x + B.slab);
    double* part = (double*)(x + B.part);
    float* dl[4];
    for (int lv = 0; lv < 4; ++lv) dl[lv] = (float*)(x + B.dl[lv]);
    const int H = g.h[0], W = g.w[0];
    const int64_t M = g.m[0];

    hipLaunchKernelGGL(fpn_train_pack_dgrad_weights_kernel, dim3(blocks_for(256 * 2304 + 256)), dim3(FT_THREADS), 0, s, (const float*)params->layer_w, wd3,
                       zero);
    // ---- dP2: bias gradient, scale, fp16 operands (flat and ring-padded)
    {
        const int G = red_blocks(M);
        hipLaunchKernelGGL(fpn_train_reduce_kernel, dim3(G), dim3(FT_THREADS), 0, s, dp2, M, rows_per_block(M, G), part, pmax);
        hipLaunchKernelGGL(fpn_train_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (const float*)pmax, G, dscale, grads->layer_b, sc);
        hipLaunchKernelGGL(fpn_train_zero_ring_kernel, dim3(blocks_for((int64_t)n * (2 * (W + 2) + 2 * H) * 32)), dim3(FT_THREADS), 0, s, dp2p, n, H, W);
        hipLaunchKernelGGL(fpn_train_form_kernel, dim3(blocks_for(M * 32)), dim3(FT_THREADS), 0, s, dp2, M, (const float*)sc, H, W, ah, dp2p);
        VTD_HIP_CHECK(hipGetLastError());
    }
    {   // ---- conv 3x3 weight gradient
        WgArgs wa;
        wa.a = ah; wa.lda = 256; wa.x = l2; wa.xc = 256; wa.n = n; wa.H = H; wa.W = W; wa.rows = M; wa.slab = slab;
        const int S = wgrad_slabs(M, true);
        wa.slab_len = slab_rows(M, S);
        hipLaunchKernelGGL(dbhead_train_wgrad_kernel<0>, dim3(18 * S, 2), dim3(WG_THREADS), 0, s, wa);
        hipLaunchKernelGGL(fpn_train_wgrad_reduce_kernel<true>, dim3(blocks_for(256 * 2304)), dim3(FT_THREADS), 0, s, (const float*)slab, S, 256 * 2304,
                           (const float*)sc, grads->layer_w);
        VTD_HIP_CHECK(hipGetLastError());
    }
    {   // ---- dL2 = conv3x3^T(dP2), at dP2's total scale
        ConvParams c = base_conv();
        c.in = dp2p; c.wgt = wd3; c.bias = zero; c.out = dl[0]; c.ldc = 256; c.flags = EPI_OUT_F32;
        c.cin_steps = 4; c.kw = 3; c.s_step = 256; c.r_step = (W + 2) * 256;
        c.M = (int)M; c.K = 2304; c.cout = 256; c.cout_pad = 256; c.ho = H; c.wo = W;
        c.in_hp = H + 2; c.in_wp = W + 2; c.in_c = 256; c.in_y0 = 0; c.in_x0 = 0;
        if ((rc = vtd_launch_conv(c, -1, s))) return rc;
    }
    // ---- the four levels, finest first
    for (int lv = 0; lv < 4; ++lv) {
        const int h = g.h[lv], w = g.w[lv], Cc = g.c[lv];
        const int64_t m = g.m[lv];
        float* scl = sc + 4 * (lv + 1);
        if (lv) hipLaunchKernelGGL(fpn_train_sumpool_kernel, dim3(blocks_for(m * 64)), dim3(FT_THREADS), 0, s, (const float*)dl[lv - 1], n, h, w, dl[lv]);
        const int G = red_blocks(m);
        hipLaunchKernelGGL(fpn_train_reduce_kernel, dim3(G), dim3(FT_THREADS), 0, s, (const float*)dl[lv], m, rows_per_block(m, G), part, pmax);
        hipLaunchKernelGGL(fpn_train_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (const float*)pmax, G, (const float*)sc,
                           grads->inner_b[3 - lv], scl);
        hipLaunchKernelGGL(fpn_train_form_kernel, dim3(blocks_for(m * 32)), dim3(FT_THREADS), 0, s, (const float*)dl[lv], m, (const float*)scl, h, w, ah,
                           (half_t*)nullptr);
        WgArgs wa;
        wa.a = ah; wa.lda = 256; wa.x = (const half_t*)taps[lv]; wa.xc = Cc; wa.n = n; wa.H = h; wa.W = w; wa.rows = m; wa.slab = slab;
        const int S = wgrad_slabs(m, false);
        wa.slab_len = slab_rows(m, S);
        hipLaunchKernelGGL(dbhead_train_wgrad_kernel<2>, dim3((Cc + 127) / 128 * S, 2), dim3(WG_THREADS), 0, s, wa);
        hipLaunchKernelGGL(fpn_train_wgrad_reduce_kernel<false>, dim3(blocks_for(256 * Cc)), dim3(FT_THREADS), 0, s, (const float*)slab, S, 256 * Cc,
                           (const float*)scl, grads->inner_w[3 - lv]);
        VTD_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// dC(k) = dL(k) inner_w[5-k] for the levels of `mask` (bit lv = C(2 + lv)), from what vtd_launch_fpn_backward left in `scratch`
int vtd_launch_fpn_backward_input(int n, int h5, int w5, int c5, const vtd_fpn_params* params, void* scratch, int mask, float* const* dtaps,
                                  float* dscale, hipStream_t s) {
    Geo g;
    if (!params || !scratch || !dtaps || !dscale || mask < 1 || mask > 15 || !make_geo(n, h5, w5, c5, g)) return -2902;
    for (int lv = 0; lv < 4; ++lv)
        if ((mask >> lv) & 1)
            if (!dtaps[lv] || !params->inner_w[3 - lv] || ((uintptr_t)params->inner_w[3 - lv] & 3)) return -2902;
    if (((uintptr_t)scratch & 255) || ((uintptr_t)dscale & 7)) return -2903;
    for (int lv = 0; lv < 4; ++lv)
        if (((mask >> lv) & 1) && ((uintptr_t)dtaps[lv] & 15)) return -2903;
    const BwdLayout B = bwd_layout(g);
    const InLayout I = in_layout(g);
    char* x = (char*)scratch;
    half_t* ah = (half_t*)(x + B.ah);
    const float* sc = (const float*)(x + B.sc);
    float* zero = (float*)(x + I.zero);
    int rc;
    for (int lv = 0; lv < 4; ++lv) {
        if (!((mask >> lv) & 1)) continue;
        const int h = g.h[lv], w = g.w[lv], Cc = g.c[lv];
        const int64_t m = g.m[lv];
        half_t* wt = (half_t*)(x + I.wt[lv]);
        hipLaunchKernelGGL(fpn_train_pack_input_weights_kernel, dim3(blocks_for((int64_t)256 * Cc + Cc)), dim3(FT_THREADS), 0, s,
                           (const float*)params->inner_w[3 - lv], Cc, wt, zero);
        // the operand the level's weight gradient read, formed again (the backward's `ah` holds the last level only)
        hipLaunchKernelGGL(fpn_train_form_kernel, dim3(blocks_for(m * 32)), dim3(FT_THREADS), 0, s, (const float*)(x + B.dl[lv]), m, sc + 4 * (lv + 1), h, w,
                           ah, (half_t*)nullptr);
        VTD_HIP_CHECK(hipGetLastError());
        ConvParams c = base_conv();   // a 1x1 convolution over the flat [n][h][w][256] operand (no ring)
        c.in = ah; c.wgt = wt; c.bias = zero; c.out = dtaps[lv]; c.ldc = Cc; c.flags = EPI_OUT_F32;
        c.cin_steps = 4; c.kw = 1; c.s_step = 256; c.r_step = w * 256;
        c.M = (int)m; c.K = 256; c.cout = Cc; c.cout_pad = Cc; c.ho = h; c.wo = w;
        c.in_hp = h; c.in_wp = w; c.in_c = 256; c.in_y0 = 0; c.in_x0 = 0;
        if ((rc = vtd_launch_conv(c, -1, s))) return rc;
    }
    hipLaunchKernelGGL(fpn_train_copy_scales_kernel, dim3(1), dim3(64), 0, s, sc, mask, dscale);
    return -(int)hipGetLastError();
}
