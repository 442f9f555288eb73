// ResNet stem training with frozen-statistics BatchNorm (the running statistics normalise and are never written; gamma and beta learn),
// forward and backward: pool = maxpool3x3/s2/p1(relu(bn(conv7x7/s2/p3(x)))) on x [n,3,H,W], H and W even.  hc x wc = H/2 x W/2 is the conv
// map, hp x wp = ceil(hc/2) x ceil(wc/2) the pooled map.  No gradient of the image is formed.
//
//   pack             NCHW fp32 / fp16 -> the stem's input layout [n][H+6][W+6][4] fp16: ring 3, a zero fourth channel, a zero ring
// Forward:
//   fold             half(w gamma rstd) into the fragment layout of stem_pool.hip ([7 ky][4 cout tiles][64 lanes][8]), bias = beta - mean gamma
//                    rstd; on the device, every call
//   forward          one launch, stem_pool.hip's tiling without its persistent LDS-DMA ring: a workgroup owns 7x8 pooled pixels = 15x17
//                    conv outputs, stages the 37x40-pixel patch in LDS with plain loads, walks K as 7 kernel rows x (8 taps x 4 ch) with the
//                    28 weight fragments in registers, writes conv + bias + ReLU as fp16 to LDS (0 outside the conv map) and pools from
//                    there: the pooled padded tap [n][hp+2][wp+2][64] and one byte per pooled element idx[n][hp][wp][64] = 3 ky + kx of the
//                    FIRST maximum of the window in scan order (ky, then kx).  The scan keeps a later position only when it is strictly
//                    greater, so where the pooled value is positive the winner is an in-image position (the others hold 0); where it is 0
//                    the byte is unspecified and the backward does not route.  The conv map never reaches HBM
// Backward from dpool (NHWC fp32 times a power of two, what vtd_block64_train_backward leaves as dx):
//   reduce / finish  m = dpool (pool > 0) at pooled resolution, formed on the fly.  Every live pooled element routes to one conv position
//                    whose ReLU is active, so the channel sums of dZ are the channel sums of m: dbeta.  Order (rb_reduce64_kernel's): at most
//                    256 workgroups of `per` consecutive pooled pixels; quarter k = t / 64 sums rows ceil(k r / 4) .. ceil((k + 1) r / 4) - 1
//                    of the workgroup's r rows in row order in fp64, the partial is (q0 + q1) + (q2 + q3), the partials are added in
//                    workgroup order.  The multiplier is a power of two from max |m| with a factor 4 of headroom under the other stages'
//                    target: a conv position can receive up to four windows
//   form             dZ [n hc wc][64] fp16 by gather: conv pixel (y, x) belongs to the windows py in {y/2} (y even) or {(y-1)/2, (y+1)/2}
//                    (y odd), columns alike: 1, 2 or 4 windows, added in (py, px) order; it takes m times the multiplier of each window
//                    whose idx names it.  Nothing is scattered
//   wgrad            G[c][q] = sum_rows dZ[row][c] X[row][q] on v_mfma_f32_16x16x32_f16, q = 32 ky + 4 kx + ci with kx < 8: X[row][32 ky ..
//                    32 ky + 31] is the 64 contiguous bytes of the image tap at pixel (2y + ky, 2x).  A kernel of its own rather than a mode
//                    of wgrad_mfma.h: that header's q-tile is 128 columns decoded as (tap, 64 or 128 channels) of a ring-1 tensor, here
//                    the whole K is one 224-column tile decoded as (ky, 64-byte row) of a ring-3 four-channel tensor, and the 64 x 224
//                    output is one workgroup's (wave w: channels 16 w .. 16 w + 15, 14 column fragments).  Slabs: min(512, ceil(rows /
//                    1024)) slabs of ceil(rows / slabs) rows rounded up to the 32-row chunk; slab [64][224] fp32
//   param            slabs summed in slab order in fp64; dW = gamma rstd G (the eighth pixel and the fourth channel dropped: 147 of 224
//                    columns), dbeta = s, dgamma = rstd (sum_k w G - mean s): no division by gamma
// No atomics, shape-only grids, fixed summation orders: bitwise repeatable.
//
// The same stage with batch-statistics BatchNorm (torch's train() mode) behind the vtd_stem_bn_train_* entries, in the second half of this
// file; training = 0 hands the call to the launches above.  The statistics need the whole conv map before anything is normalised, so z
// [n hc wc][64] fp32 makes one round trip through HBM per direction:
//   pack             half(w) into fold's fragment layout: no gamma rstd, no bias
//   conv             the forward kernel's tiling and K walk with ZOUT: the fp32 accumulators to z, each conv pixel by the one tile that owns it
//   stats            (count, mean, M2) per channel in resblock_bn_train.hip's 64-wide order, with the channel's min and max of z; finish: Chan's
//                    combination, the running update, the table {mu, rstd, gamma, beta, max |xh|}
//   pool             a = half(relu(((z - mu) rstd) gamma + beta)) pooled straight from z by the frozen kernel's index rule; a is not stored
//   reduce / finish  s1 = sum m and s2 = sum m xh[the position idx names] at pooled resolution in st_reduce_kernel's row order; dbeta, dgamma,
//                    coef = {gamma rstd, s1 / M, s2 / M} with M the conv rows, the power-of-two multiplier
//   form             dZ = gamma rstd (g - s1 / M - xh s2 / M), g gathered by st_form_kernel's membership rule, dense fp16
//   wgrad / dw       stem_train_wgrad_kernel unchanged; dW = G / scale
#include "vtd_common.h"
#include "../../include/vtd.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_MAX_RED = 256;
constexpr float ST_SCALE_TARGET = 4096.0f;   // the block kernels' 16384 / 4: up to four windows add into one conv position
constexpr int ST_ARG = -3301, ST_ALIGN = -3302;

constexpr int ST_PT_ROWS = 7, ST_PT_COLS = 8;        // pooled pixels per tile
constexpr int ST_CT_COLS = 17;                       // conv outputs per tile: 15 rows x 17 columns (255 of the 256 GEMM rows)
constexpr int ST_PATCH_COLS = 40, ST_PATCH_ROWS = 37; // staged input patch (the idle 256th GEMM row reads rows 30 .. 36)
constexpr int ST_PATCH_BYTES = ST_PATCH_ROWS * ST_PATCH_COLS * 8;
constexpr int ST_CT_PITCH = 144;                     // bytes per conv pixel in LDS (64 ch fp16 + 16 pad)
constexpr int ST_WFRAG = 7 * 4 * 64 * 8;             // halfs of the folded fragment image

constexpr int SW_KC = 32;                            // rows per K chunk of the weight gradient
constexpr int SW_P = 64, SW_Q = 224;

typedef short short8v __attribute__((ext_vector_type(8)));

inline int64_t a256(int64_t x) { return (x + 255) & ~(int64_t)255; }
inline unsigned nblk(int64_t items) { return (unsigned)((items + ST_THREADS - 1) / ST_THREADS); }

struct Geo {
    int n, H, W, hc, wc, hp, wp;
    int64_t mc, mp;   // conv pixels, pooled pixels
};

bool make_geo(int n, int H, int W, Geo& g) {
    if (n <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1) || n > 65535 || H > 8192 || W > 8192) return false;
    g.n = n; g.H = H; g.W = W; g.hc = H / 2; g.wc = W / 2; g.hp = (g.hc + 1) / 2; g.wp = (g.wc + 1) / 2;
    g.mc = (int64_t)n * g.hc * g.wc; g.mp = (int64_t)n * g.hp * g.wp;
    return g.mc * 64 < (1ll << 31) && (int64_t)n * (H + 6) * (W + 6) * 4 < (1ll << 31);
}

inline int wg_slabs(int64_t rows) { const int64_t s = (rows + 1023) / 1024; return (int)(s < 1 ? 1 : s > 512 ? 512 : s); }
inline int64_t slab_rows(int64_t rows, int s) { return ((rows + s - 1) / s + SW_KC - 1) / SW_KC * SW_KC; }

struct FwdLayout { int64_t w, bias, total; };
struct BwdLayout { int64_t dz, part, pmax, sum, sc, slab, total; };

FwdLayout fwd_layout() {
    FwdLayout L;
    L.w = 0; L.bias = a256(ST_WFRAG * 2); L.total = L.bias + a256(64 * 4);
    return L;
}

BwdLayout bwd_layout(const Geo& g) {
    BwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    L.dz = take(g.mc * 64 * 2);
    L.part = take((int64_t)ST_MAX_RED * 64 * 8); L.pmax = take(ST_MAX_RED * 4);
    L.sum = take(64 * 8); L.sc = take(4 * 4);
    L.slab = take((int64_t)wg_slabs(g.mc) * SW_P * SW_Q * 4);
    L.total = o;
    return L;
}

// MFMA row fr of cout tile i carries this output channel (stem_pool.hip: sp_chan)
__host__ __device__ constexpr int st_chan(int tile, int row) { return 32 * (tile >> 1) + 8 * (row >> 2) + 4 * (tile & 1) + (row & 3); }

// ---- pack ---------------------------------------------------------------------------------------------------------------------------------
// One thread = one pixel of the padded tap: the three channels of an in-image pixel, zeros elsewhere.
template <typename T>
__global__ __launch_bounds__(ST_THREADS) void st_pack_kernel(const T* x, int n, int H, int W, half_t* tap) {
    const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    const int Hp = H + 6, Wp = W + 6;
    if (i >= (int64_t)n * Hp * Wp) return;
    const int xp = (int)(i % Wp);
    const int64_t q = i / Wp;
    const int yp = (int)(q % Hp), img = (int)(q / Hp);
    half4 v = {0, 0, 0, 0};
    if (yp >= 3 && yp < H + 3 && xp >= 3 && xp < W + 3) {
        const int64_t plane = (int64_t)H * W, o = (int64_t)img * 3 * plane + (int64_t)(yp - 3) * W + (xp - 3);
        v[0] = (half_t)x[o]; v[1] = (half_t)x[o + plane]; v[2] = (half_t)x[o + 2 * plane];
    }
    *(half4*)(tap + i * 4) = v;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
// wfrag [7 ky][4 tiles][64 lanes][8]: lane (fr, fq) of tile i holds half(w[co][c][ky][kx] gamma rstd) for co = st_chan(i, fr), kx = 2 fq +
// (e >> 2), c = e & 3 (zero for kx = 7 and c = 3); bias[co] = beta - mean gamma rstd
__global__ __launch_bounds__(ST_THREADS) void st_fold_kernel(const float* w, const float* gam, const float* bet, const float* mean, const float* var,
                                                             float eps, half_t* wfrag, float* bias) {
    const int i = blockIdx.x * ST_THREADS + threadIdx.x;
    if (i < ST_WFRAG) {
        const int e = i & 7, lane = (i >> 3) & 63, tile = (i >> 9) & 3, ky = i >> 11;
        const int fr = lane & 15, fq = lane >> 4, co = st_chan(tile, fr), kx = 2 * fq + (e >> 2), c = e & 3;
        float v = 0.f;
        if (kx < 7 && c < 3) v = w[((co * 3 + c) * 7 + ky) * 7 + kx] * (gam[co] / sqrtf(var[co] + eps));
        wfrag[i] = (half_t)v;
    } else if (i < ST_WFRAG + 64) {
        const int co = i - ST_WFRAG;
        bias[co] = bet[co] - mean[co] * (gam[co] / sqrtf(var[co] + eps));
    }
}

// the one-pixel ring of the pooled padded tap.  One thread = 8 channels of one ring pixel.
__global__ __launch_bounds__(ST_THREADS) void st_zero_ring_kernel(half_t* t, int n, int H, int Wd) {
    const int Hp = H + 2, Wp = Wd + 2, R = 2 * Wp + 2 * H;
    const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= (int64_t)n * R * 8) return;
    const int c8 = (int)(i & 7);
    const int64_t q = i >> 3;
    const int r = (int)(q % R), img = (int)(q / R);
    int yp, xp;
    if (r < Wp) { yp = 0; xp = r; }
    else if (r < 2 * Wp) { yp = Hp - 1; xp = r - Wp; }
    else { const int k = r - 2 * Wp; yp = 1 + (k >> 1); xp = (k & 1) ? Wp - 1 : 0; }
    const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    *(half8*)(t + (((int64_t)img * Hp + yp) * Wp + xp) * 64 + c8 * 8) = z;
}

struct StemFwdParams {
    const half_t* in;    // [n][in_hp][in_wp][4] fp16, ring 3
    const half_t* w;     // the fragment image of st_fold_kernel
    const float* bias;   // [64]
    half_t* out;         // [n][pool_h + 2][pool_w + 2][64], ring 1
    uint8_t* idx;        // [n][pool_h][pool_w][64]
    float* z;            // ZOUT: [n conv_h conv_w][64] fp32, the raw convolution (no bias, no activation, nothing pooled)
    int n, in_hp, in_wp, conv_h, conv_w, pool_h, pool_w, tiles_x, tiles_y;
};

// ZOUT (the batch-statistics forward): the same patch, fragments and K walk on raw fp16 weights from zero accumulators; the fp32 accumulators
// go to p.z and nothing else is written.  Neighbouring tiles share one conv row and one conv column, so a tile writes its local rows 1 .. 14
// and columns 1 .. 16 only: conv pixel (y, x) belongs to tile (y / 14, x / 16) and to no other.
template <bool ZOUT>
__global__ __launch_bounds__(ST_THREADS, 2) void stem_train_forward_kernel(const StemFwdParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[ZOUT ? ST_PATCH_BYTES : ST_PATCH_BYTES + 256 * ST_CT_PITCH + 256];
    unsigned char* const patch = smem;                                   // [37][40] pixels of 8 bytes
    unsigned char* const ctile = smem + ST_PATCH_BYTES;                  // [256][ST_CT_PITCH]
    float* const bias_lds = (float*)(ctile + 256 * ST_CT_PITCH);         // [64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    const int per_img = p.tiles_x * p.tiles_y;
    const int img = blockIdx.x / per_img, r = blockIdx.x - img * per_img, ty = r / p.tiles_x;
    const int py0 = ty * ST_PT_ROWS, px0 = (r - ty * p.tiles_x) * ST_PT_COLS;

    half8 wreg[7][4];
#pragma unroll
    for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int i = 0; i < 4; ++i) wreg[ky][i] = *(const half8*)(p.w + ((ky * 4 + i) * 64 + lane) * 8);
    if constexpr (!ZOUT) {
        if (tid < 64) bias_lds[tid] = p.bias[tid];
    }
    // The patch: input rows 4 py0 - 2 .., columns 4 px0 - 2 .., in units of two pixels (16 bytes; the tap's row pitch is even).  Coordinates
    // outside the padded image are clamped, not zero-filled: such pixels only feed conv outputs outside the conv map, which the epilogue
    // replaces by 0, or the zero weights of the eighth tap -- and what is read instead is a finite fp16 of the same tensor.
    {
        const half_t* base = p.in + (int64_t)img * p.in_hp * p.in_wp * 4;
        for (int u = tid; u < ST_PATCH_ROWS * (ST_PATCH_COLS / 2); u += ST_THREADS) {
            const int row = u / (ST_PATCH_COLS / 2), col = 2 * (u - row * (ST_PATCH_COLS / 2));
            int iy = 4 * py0 - 2 + row, ix = 4 * px0 - 2 + col;
            iy = iy < 0 ? 0 : iy > p.in_hp - 1 ? p.in_hp - 1 : iy;
            ix = ix < 0 ? 0 : ix > p.in_wp - 2 ? p.in_wp - 2 : ix;
            *(half8*)(patch + u * 16) = *(const half8*)(base + ((int64_t)iy * p.in_wp + ix) * 4);
        }
    }
    // this lane's four GEMM rows (conv pixels of the tile) -> LDS byte offset of tap (ky = 0, kx = 2 fq)
    int a_off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pix = wv * 64 + j * 16 + fr;
        const int c_row = pix / ST_CT_COLS, c_col = pix - c_row * ST_CT_COLS;
        a_off[j] = ((2 * c_row) * ST_PATCH_COLS + 2 * c_col + 2 * fq) * 8;
    }
    __syncthreads();

    floatx4 acc[4][4];  // [cout tile][pixel fragment]; the BN shift rides in the accumulator
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (ZOUT) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
            else acc[i][j] = *(const floatx4*)(bias_lds + st_chan(i, fq * 4));
        }
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
        half8 af[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] = *(const half8*)(patch + a_off[j] + ky * (ST_PATCH_COLS * 8));
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wreg[ky][i], af[j], acc[i][j], 0, 0, 0);
    }

    if constexpr (ZOUT) {
        // lane (fr, fq) holds channels 32 k + 8 fq .. + 7 of its pixel in the accumulators of the tile pair (2k, 2k + 1): 32 contiguous bytes
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pix = wv * 64 + j * 16 + fr;
            const int c_row = pix / ST_CT_COLS, c_col = pix - c_row * ST_CT_COLS;
            const int cy = 2 * py0 - 1 + c_row, cx = 2 * px0 - 1 + c_col;
            if (c_row < 1 || c_row > 2 * ST_PT_ROWS || c_col < 1 || c_col > 2 * ST_PT_COLS || cy >= p.conv_h || cx >= p.conv_w) continue;
            float* dst = p.z + (((int64_t)img * p.conv_h + cy) * p.conv_w + cx) * 64 + 8 * fq;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                *(floatx4*)(dst + 32 * k) = acc[2 * k][j];
                *(floatx4*)(dst + 32 * k + 4) = acc[2 * k + 1][j];
            }
        }
        return;
    }
    // ReLU after the fp16 convert (every negative half, -0 included, is a negative int16), zero outside the conv map -> LDS conv tile: lane
    // (fr, fq) holds channels 32 k + 8 fq .. + 7 of its pixel in the accumulators of the tile pair (2k, 2k + 1)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pix = wv * 64 + j * 16 + fr;
        const int c_row = pix / ST_CT_COLS, c_col = pix - c_row * ST_CT_COLS;
        const int cy = 2 * py0 - 1 + c_row, cx = 2 * px0 - 1 + c_col;
        const bool valid = cy >= 0 && cy < p.conv_h && cx >= 0 && cx < p.conv_w;
        unsigned char* dst = ctile + pix * ST_CT_PITCH + fq * 16;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const floatx4 a = acc[2 * k][j], b = acc[2 * k + 1][j];
            half8 hv = half8{(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3], (half_t)b[0], (half_t)b[1], (half_t)b[2], (half_t)b[3]};
            hv = __builtin_bit_cast(half8, __builtin_elementwise_max(__builtin_bit_cast(short8v, hv), short8v{0, 0, 0, 0, 0, 0, 0, 0}));
            if (!valid) hv = half8{0, 0, 0, 0, 0, 0, 0, 0};
            *(half8*)(dst + k * 64) = hv;
        }
    }
    __syncthreads();

    // 3x3/s2 max over the conv tile with the position of the first maximum: item = (pooled pixel, 8-channel group); a wave's 64 items are
    // one pooled row (8 pixels x 8 groups, stem_pool.hip's lane assignment), waves 0..2 own two rows.  Post-ReLU fp16 values are >= +0, so
    // their bit patterns order like int16
    const int cg = (lane >> 2) & 7;
    const int qx = ((lane >> 5) & 1) | ((lane & 3) << 1);
    const int px = px0 + qx;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (it == 1 && wv == 3) break;
        const int prow = wv + 4 * it, py = py0 + prow;
        const unsigned char* src = ctile + ((2 * prow) * ST_CT_COLS + 2 * qx) * ST_CT_PITCH + cg * 16;
        short8v m = *(const short8v*)src;
        short8v id = short8v{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 1; q < 9; ++q) {
            const short8v v = *(const short8v*)(src + ((q / 3) * ST_CT_COLS + (q % 3)) * ST_CT_PITCH);
            const short8v gt = v > m;                  // all ones where strictly greater: an earlier position keeps a tie
            m = (gt & v) | (~gt & m);
            id = (gt & (short)q) | (~gt & id);
        }
        if (py < p.pool_h && px < p.pool_w) {
            *(short8v*)(p.out + (((int64_t)img * (p.pool_h + 2) + py + 1) * (p.pool_w + 2) + px + 1) * 64 + cg * 8) = m;
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) { lo |= (uint32_t)(id[e] & 0xff) << (8 * e); hi |= (uint32_t)(id[4 + e] & 0xff) << (8 * e); }
            *(uint2*)(p.idx + (((int64_t)img * p.pool_h + py) * p.pool_w + px) * 64 + cg * 8) = make_uint2(lo, hi);
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------
// m[row][c] = dpool[row][c] where the pooled tap at pixel `row` is positive, else 0, summed per channel in rb_reduce64_kernel's order (the
// head of this file): part[g][64] fp64, pmax[g]
__global__ __launch_bounds__(ST_THREADS) void st_reduce_kernel(const float* dpool, const half_t* pool, int64_t rows, int64_t per, int hp, int wp, double* part,
                                                               float* pmax) {
    const int t = threadIdx.x, c = t & 63, k = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t r = m1 - m0, lo = m0 + (k * r + 3) / 4, hi = m0 + ((k + 1) * r + 3) / 4;
    const int HW = hp * wp;
    double s = 0.0;
    float mx = 0.f;
    if (lo < hi) {
        int img = (int)(lo / HW), rem = (int)(lo - (int64_t)img * HW), y = rem / wp, x = rem - y * wp;
        for (int64_t m = lo; m < hi; ++m) {
            const bool live = (float)pool[(((int64_t)img * (hp + 2) + y + 1) * (wp + 2) + x + 1) * 64 + c] > 0.f;
            const float a = live ? dpool[m * 64 + c] : 0.f, fa = fabsf(a);
            s += (double)a;
            mx = fa > mx || fa != fa ? fa : mx;
            if (++x == wp) { x = 0; if (++y == hp) { y = 0; ++img; } }
        }
    }
    __shared__ double shs[ST_THREADS];
    __shared__ float shm[ST_THREADS];
    shs[t] = s;
    shm[t] = mx;
    __syncthreads();
    if (k == 0) part[(int64_t)blockIdx.x * 64 + c] = (shs[c] + shs[64 + c]) + (shs[128 + c] + shs[192 + c]);
    if (t == 0) {
        float v = shm[0];
        for (int j = 1; j < ST_THREADS; ++j) v = shm[j] > v || shm[j] != shm[j] ? shm[j] : v;
        pmax[blockIdx.x] = v;
    }
}

// partials in workgroup order: sum[c] = the channel sum with the incoming scale undone (fp64); out_sc = {total scale, 1 / total, this
// stage's multiplier, 0}, the multiplier a power of two from max |m| (1 when that is zero or not finite)
__global__ __launch_bounds__(64) void st_finish_kernel(const double* part, const float* pmax, int G, const float* in_sc, double* sum, float* out_sc) {
    const int c = threadIdx.x;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(int64_t)g * 64 + c];
    sum[c] = s * (double)in_sc[1];
    if (c == 0) {
        float mx = pmax[0];
        for (int g = 1; g < G; ++g) mx = pmax[g] > mx || pmax[g] != pmax[g] ? pmax[g] : mx;
        const double tin = (double)in_sc[0];
        int e = 0;
        if (mx > 0.f && isfinite(mx)) e = (int)floor(log2((double)ST_SCALE_TARGET / (double)mx));
        const int ein = (tin > 0.0 && isfinite(tin)) ? ilogb(tin) : 0;
        int et = ein + e;
        et = et < -120 ? -120 : et > 120 ? 120 : et;
        e = et - ein;
        const double tot = tin * ldexp(1.0, e);
        out_sc[0] = (float)tot; out_sc[1] = (float)(1.0 / tot); out_sc[2] = ldexpf(1.0f, e); out_sc[3] = 0.f;
    }
}

// dZ[row][c] for conv pixel row = (img, y, x): the sum, in (py, px) order, of m times the multiplier over the windows that hold the pixel
// and whose idx names it.  One thread = 8 channels of one conv pixel.
__global__ __launch_bounds__(ST_THREADS) void st_form_kernel(const float* dpool, const half_t* pool, const uint8_t* idx, const float* sc, int64_t rows, int hc,
                                                             int wc, int hp, int wp, half_t* dz) {
    const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= rows * 8) return;
    const int c8 = (int)(i & 7);
    const int64_t m = i >> 3;
    const int HW = hc * wc, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / wc, x = rem - y * wc;
    const float mul = sc[2];
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int py0 = y >> 1, py1 = (y + 1) >> 1, px0 = x >> 1, px1 = (x + 1) >> 1;
    for (int py = py0; py <= py1 && py < hp; ++py)
        for (int px = px0; px <= px1 && px < wp; ++px) {
            const int code = 3 * (y - 2 * py + 1) + (x - 2 * px + 1);
            const int64_t pp = ((int64_t)img * hp + py) * wp + px;
            const uint2 ib = *(const uint2*)(idx + pp * 64 + c8 * 8);
            const half8 pv = *(const half8*)(pool + (((int64_t)img * (hp + 2) + py + 1) * (wp + 2) + px + 1) * 64 + c8 * 8);
            const floatx4 d0 = *(const floatx4*)(dpool + pp * 64 + c8 * 8), d1 = *(const floatx4*)(dpool + pp * 64 + c8 * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if ((int)((ib.x >> (8 * e)) & 0xff) == code && (float)pv[e] > 0.f) acc[e] += d0[e] * mul;
                if ((int)((ib.y >> (8 * e)) & 0xff) == code && (float)pv[4 + e] > 0.f) acc[4 + e] += d1[e] * mul;
            }
        }
    half8 h;
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (half_t)acc[e];
    *(half8*)(dz + i * 8) = h;
}

struct StemWgArgs {
    const half_t* dz;   // [rows][64]
    const half_t* x;    // [n][in_hp][in_wp][4]
    int hc, wc, in_hp, in_wp;
    int64_t rows, slab_len;
    float* slab;        // [slabs][64][224]
};

// Workgroup = 4 waves, one slab, the whole 64 x 224 output: wave w owns channels 16 w .. 16 w + 15 and the 14 column fragments.  Per K
// chunk of 32 rows a thread loads rows 8 o .. 8 o + 7 of one column pair of dZ (128 slots) and of X (448 slots: two per thread) with
// 4-byte loads, the next chunk's in flight during this chunk's MFMAs, and transposes them into LDS as [row octet][column][8] so that a
// fragment (8 consecutive rows of one column) is one 16-byte read; double-buffered, one barrier per chunk.  Rows past the slab load zeros.
__global__ __launch_bounds__(ST_THREADS) void stem_train_wgrad_kernel(const StemWgArgs A) {
    __shared__ __attribute__((aligned(16))) half_t lds[2][4 * (SW_P + SW_Q) * 8];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, sl = blockIdx.x;
    const int64_t r0 = (int64_t)sl * A.slab_len;
    const int64_t r1 = r0 + A.slab_len < A.rows ? r0 + A.slab_len : A.rows;
    const int nchunks = r1 > r0 ? (int)((r1 - r0 + SW_KC - 1) / SW_KC) : 0;

    const int ap = t % (SW_P / 2), ao = t / (SW_P / 2);
    const bool a_act = ao < 4;
    int bp[2], bo[2], boff[2];   // X slot s: column pair bp of octet bo; its 4 bytes sit boff halfs into kernel row bky's 64-byte run
    int bky[2];
    bool b_act[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int slot = t + s * ST_THREADS;
        b_act[s] = slot < 4 * (SW_Q / 2);
        bp[s] = slot % (SW_Q / 2); bo[s] = b_act[s] ? slot / (SW_Q / 2) : 0;
        bky[s] = (2 * bp[s]) >> 5; boff[s] = (2 * bp[s]) & 31;
    }
    const int HW = A.hc * A.wc;

    uint32_t ra[8], rb[2][8];
    auto gload = [&](int ch) {
        const int64_t base = r0 + (int64_t)ch * SW_KC;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t m = base + 8 * ao + j;
            ra[j] = (a_act && m < r1) ? *(const uint32_t*)(A.dz + m * 64 + 2 * ap) : 0u;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int64_t m = base + 8 * bo[s];
            int img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / A.wc, xx = rem - y * A.wc;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                rb[s][j] = (b_act[s] && m < r1)
                               ? *(const uint32_t*)(A.x + (((int64_t)img * A.in_hp + 2 * y + bky[s]) * A.in_wp + 2 * xx) * 4 + boff[s])
                               : 0u;
                ++m;
                if (++xx == A.wc) { xx = 0; if (++y == A.hc) { y = 0; ++img; } }
            }
        }
    };
    auto lstore = [&](int buf) {
        half_t* la = lds[buf];
        half_t* lb = lds[buf] + 4 * SW_P * 8;
        if (a_act) {
            half8 lo, hi;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lo[j] = __builtin_bit_cast(half2v, ra[j])[0];
                hi[j] = __builtin_bit_cast(half2v, ra[j])[1];
            }
            *(half8*)(la + (ao * SW_P + 2 * ap) * 8) = lo;
            *(half8*)(la + (ao * SW_P + 2 * ap + 1) * 8) = hi;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!b_act[s]) continue;
            half8 lo, hi;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lo[j] = __builtin_bit_cast(half2v, rb[s][j])[0];
                hi[j] = __builtin_bit_cast(half2v, rb[s][j])[1];
            }
            *(half8*)(lb + (bo[s] * SW_Q + 2 * bp[s]) * 8) = lo;
            *(half8*)(lb + (bo[s] * SW_Q + 2 * bp[s] + 1) * 8) = hi;
        }
    };

    floatx4 acc[SW_Q / 16];
#pragma unroll
    for (int j = 0; j < SW_Q / 16; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};

    if (nchunks > 0) gload(0);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        lstore(buf);
        __syncthreads();
        if (ch + 1 < nchunks) gload(ch + 1);
        const half_t* la = lds[buf];
        const half_t* lb = lds[buf] + 4 * SW_P * 8;
        const int oct = lane >> 4, col = lane & 15;
        const half8 fa = *(const half8*)(la + (oct * SW_P + w * 16 + col) * 8);
#pragma unroll
        for (int j = 0; j < SW_Q / 16; ++j) {
            const half8 fb = *(const half8*)(lb + (oct * SW_Q + j * 16 + col) * 8);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, fb, acc[j], 0, 0, 0);
        }
    }

    // C row c = 16 w + 4 (lane >> 4) + e, column q = 16 j + (lane & 15)
    float* out = A.slab + (int64_t)sl * SW_P * SW_Q;
#pragma unroll
    for (int j = 0; j < SW_Q / 16; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) out[(w * 16 + 4 * (lane >> 4) + e) * SW_Q + j * 16 + (lane & 15)] = acc[j][e];
}

// One workgroup per output channel c, thread k < 147 = (ci, ky, kx) in the weight's own order.  G = the slabs summed in slab order (fp64)
// with the scale undone, read at column 32 ky + 4 kx + ci; dW = gamma rstd G; dbeta = s; dgamma = rstd (sum_k w G - mean s), the sum in
// fp64 in a fixed tree order
__global__ __launch_bounds__(ST_THREADS) void st_param_kernel(const float* slab, int S, const float* sc, const double* sum, const float* w, const float* gam,
                                                              const float* mean, const float* var, float eps, float* dw, float* dgam, float* dbet) {
    const int c = blockIdx.x, t = threadIdx.x;
    const double rstd = 1.0 / sqrt((double)var[c] + (double)eps), inv = (double)sc[1], f = (double)gam[c] * rstd;
    double dot = 0.0;
    if (t < 147) {
        const int ci = t / 49, ky = (t % 49) / 7, kx = t % 7, q = 32 * ky + 4 * kx + ci;
        double G = 0.0;
        for (int s = 0; s < S; ++s) G += (double)slab[((int64_t)s * SW_P + c) * SW_Q + q];
        G *= inv;
        dw[c * 147 + t] = (float)(f * G);
        dot = (double)w[c * 147 + t] * G;
    }
    __shared__ double sh[ST_THREADS];
    sh[t] = dot;
    __syncthreads();
    for (int o = ST_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) {
        dgam[c] = (float)(rstd * (sh[0] - (double)mean[c] * sum[c]));
        dbet[c] = (float)sum[c];
    }
}

// ---- batch-statistics BatchNorm (training = 1) --------------------------------------------------------------------------------------------
// The conventions of resblock_bn_train.hip at width 64: raw weights rounded to fp16 per call, z kept in fp32, fixed fp64 summation orders.

constexpr int SB_ARG = -3801, SB_ALIGN = -3802;
constexpr float SB_SCALE_TARGET = 4.f * ST_SCALE_TARGET;   // the block kernels' 16384: the bound on |dz| counts the four windows itself
constexpr int SB_PARTS = 16, SB_LANES = 16;                // sixteen parts of 16 lanes x 4 channels

typedef double doublex4 __attribute__((ext_vector_type(4)));

// the workspace of a training = 1 forward.  w sits where the frozen layout keeps its folded image.  tab: {mu, rstd, gamma, beta, max |xh|} [5][64]
struct BnFwdLayout { int64_t w, tab, part, pmm, z, total; };
struct BnBwdLayout { int64_t dz, part, pmax, coef, sc, slab, total; };

BnFwdLayout bn_fwd_layout(const Geo& g) {
    BnFwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    L.w = take(ST_WFRAG * 2); L.tab = take(5 * 64 * 4);
    L.part = take((int64_t)ST_MAX_RED * 64 * 3 * 8); L.pmm = take((int64_t)ST_MAX_RED * 2 * 64 * 4);
    L.z = take(g.mc * 64 * 4);
    L.total = o;
    return L;
}

BnBwdLayout bn_bwd_layout(const Geo& g) {
    BnBwdLayout L;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    L.dz = take(g.mc * 64 * 2);
    L.part = take((int64_t)ST_MAX_RED * 2 * 64 * 8); L.pmax = take((int64_t)ST_MAX_RED * 64 * 4);
    L.coef = take(3 * 64 * 4); L.sc = take(4 * 4);
    L.slab = take((int64_t)wg_slabs(g.mc) * SW_P * SW_Q * 4);
    L.total = o;
    return L;
}

// workgroups over the M rows of z: min(256, ceil(M / 256)) of ceil(M / workgroups) consecutive rows
inline int bn_red(int64_t rows) { const int64_t r = (rows + 255) / 256; return (int)(r < 1 ? 1 : r > ST_MAX_RED ? ST_MAX_RED : r); }

// NaN-keeping maximum, as the reduce kernels above take it
__device__ __forceinline__ float st_nmax(float m, float a) { return a > m || a != a ? a : m; }

// st_fold_kernel's fragment image of the raw weights: half(w), no gamma rstd, no bias
__global__ __launch_bounds__(ST_THREADS) void sb_pack_kernel(const float* w, half_t* wfrag) {
    const int i = blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= ST_WFRAG) return;
    const int e = i & 7, lane = (i >> 3) & 63, tile = (i >> 9) & 3, ky = i >> 11;
    const int fr = lane & 15, fq = lane >> 4, co = st_chan(tile, fr), kx = 2 * fq + (e >> 2), c = e & 3;
    wfrag[i] = (half_t)((kx < 7 && c < 3) ? w[((co * 3 + c) * 7 + ky) * 7 + kx] : 0.f);
}

// the sixteen parts of one workgroup, part 0 in registers and the others in LDS [part - 1][value][lane]: the balanced pairwise tree, the
// eight-part order on q0 .. q7 and on q8 .. q15, then lower + upper (resblock_bn_train.hip: bt_join at sixteen parts)
__device__ __forceinline__ double sb_join(double own, double (*sh)[8][SB_LANES], int v, int j) {
    const double lower = ((own + sh[0][v][j]) + (sh[1][v][j] + sh[2][v][j])) + ((sh[3][v][j] + sh[4][v][j]) + (sh[5][v][j] + sh[6][v][j]));
    const double upper = ((sh[7][v][j] + sh[8][v][j]) + (sh[9][v][j] + sh[10][v][j])) + ((sh[11][v][j] + sh[12][v][j]) + (sh[13][v][j] + sh[14][v][j]));
    return lower + upper;
}

// z [rows][64] fp32 -> part[g][c] = {count, mean, M2} (fp64) in the 64-wide order of resblock_bn_train.hip (bt_stats_partial_kernel<64>):
// thread (part k = t / 16, lane j = t % 16) sums channels 4 j .. 4 j + 3 over rows ceil(k r / 16) .. ceil((k + 1) r / 16) - 1 of the
// workgroup's r rows.  The same pass takes the channel's minimum and maximum of z, pmm[g] = {min[64], max[64]}: the backward reads z at
// pooled resolution only and has max |xh| from these
__global__ __launch_bounds__(ST_THREADS) void sb_stats_partial_kernel(const float* z, int64_t rows, int64_t per, double* part, float* pmm) {
    const int t = threadIdx.x, j = t % SB_LANES, grp = t / SB_LANES;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t r = m1 - m0, lo = m0 + (grp * r + SB_PARTS - 1) / SB_PARTS, hi = m0 + ((grp + 1) * r + SB_PARTS - 1) / SB_PARTS;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    floatx4 mn = {INFINITY, INFINITY, INFINITY, INFINITY}, mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll 4
    for (int64_t m = lo; m < hi; ++m) {
        const floatx4 v = *(const floatx4*)(z + m * 64 + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double a = (double)v[e];
            s[e] += a; q[e] += a * a;
            mn[e] = fminf(mn[e], v[e]); mx[e] = fmaxf(mx[e], v[e]);
        }
    }
    __shared__ double sh[SB_PARTS - 1][8][SB_LANES];
    __shared__ float shm[SB_PARTS - 1][8][SB_LANES];
    if (grp) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sh[grp - 1][e][j] = s[e]; sh[grp - 1][4 + e][j] = q[e];
            shm[grp - 1][e][j] = mn[e]; shm[grp - 1][4 + e][j] = mx[e];
        }
    }
    __syncthreads();
    if (!grp) {
        const double cnt = (double)r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double S = sb_join(s[e], sh, e, j), Q = sb_join(q[e], sh, 4 + e, j);
            const double mean = cnt > 0 ? S / cnt : 0.0;
            double* o = part + ((int64_t)blockIdx.x * 64 + 4 * j + e) * 3;
            o[0] = cnt; o[1] = mean; o[2] = cnt > 0 ? fmax(Q - S * mean, 0.0) : 0.0;
#pragma unroll
            for (int k = 0; k < SB_PARTS - 1; ++k) { mn[e] = fminf(mn[e], shm[k][e][j]); mx[e] = fmaxf(mx[e], shm[k][4 + e][j]); }
        }
        *(floatx4*)(pmm + (int64_t)blockIdx.x * 128 + 4 * j) = mn;
        *(floatx4*)(pmm + (int64_t)blockIdx.x * 128 + 64 + 4 * j) = mx;
    }
}

// One workgroup per channel: Chan's combination of the partials in workgroup order (fp64), torch's running-statistics update with the
// unbiased variance, the table {mu, rstd, gamma, beta, max |xh|} [5][64] (xh = (z - mu) rstd in fp32, as the other kernels form it: its
// extremes sit at the extremes of z) and (optionally) stats_out = {mu, sigma^2} [2][64].  The combination is a serial chain; thread g brings
// partial g (G <= 256) into LDS first so that the chain, on thread 0, does not wait for HBM at every step
__global__ __launch_bounds__(ST_THREADS) void sb_stats_finish_kernel(const double* part, const float* pmm, int G, const float* gam, const float* bet,
                                                                     float* rmean, float* rvar, float momentum, float eps, float* tab, float* stats_out) {
    const int c = blockIdx.x, t = threadIdx.x;
    __shared__ double sp[ST_MAX_RED][3];
    __shared__ float sm[ST_MAX_RED][2];
    if (t < G) {
        const double* q = part + ((int64_t)t * 64 + c) * 3;
        sp[t][0] = q[0]; sp[t][1] = q[1]; sp[t][2] = q[2];
        sm[t][0] = pmm[(int64_t)t * 128 + c]; sm[t][1] = pmm[(int64_t)t * 128 + 64 + c];
    }
    __syncthreads();
    if (t) return;
    double n = 0.0, mu = 0.0, m2 = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int g = 0; g < G; ++g) {
        const double nb = sp[g][0];
        if (nb <= 0.0) continue;
        const double tot = n + nb, d = sp[g][1] - mu;
        mu += d * (nb / tot);
        m2 += sp[g][2] + d * d * (n * nb / tot);
        n = tot;
        mn = fminf(mn, sm[g][0]); mx = fmaxf(mx, sm[g][1]);
    }
    const double var = m2 / n, unbiased = m2 / (n - 1.0);   // n >= 2: the entry refuses fewer rows
    rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mu);
    rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * unbiased);
    const float muf = (float)mu, rs = (float)(1.0 / sqrt(var + (double)eps));
    tab[c] = muf;
    tab[64 + c] = rs;
    tab[128 + c] = gam[c];
    tab[192 + c] = bet[c];
    tab[256 + c] = fmaxf(fabsf((mn - muf) * rs), fabsf((mx - muf) * rs));
    if (stats_out) {
        stats_out[c] = muf;
        stats_out[64 + c] = (float)var;
    }
}

// a = half(relu(((z - mu) rstd) gamma + beta)) (bt_apply_kernel's expression), pooled 3x3/s2/p1 by the frozen kernel's rule: positions outside
// the conv map hold 0, the scan (ky, then kx) keeps a later position only when it is strictly greater.  One thread = 8 channels of one
// pooled pixel; a is not stored.
__global__ __launch_bounds__(ST_THREADS) void sb_pool_kernel(const float* z, const float* tab, int64_t prow, int hc, int wc, int hp, int wp, half_t* pool,
                                                             uint8_t* idx) {
    const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= prow * 8) return;
    const int c0 = (int)(i & 7) * 8;
    const int64_t m = i >> 3;
    const int HW = hp * wp, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), py = rem / wp, px = rem - py * wp;
    float mu[8], rs[8], gm[8], bt[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { mu[e] = tab[c0 + e]; rs[e] = tab[64 + c0 + e]; gm[e] = tab[128 + c0 + e]; bt[e] = tab[192 + c0 + e]; }
    half8 best;
    uint32_t id[8];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const int y = 2 * py - 1 + q / 3, x = 2 * px - 1 + q % 3;
        half8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (y >= 0 && y < hc && x >= 0 && x < wc) {
            const float* src = z + (((int64_t)img * hc + y) * wc + x) * 64 + c0;
            const floatx4 v0 = *(const floatx4*)src, v1 = *(const floatx4*)(src + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = e < 4 ? v0[e] : v1[e - 4];
                const float f = ((v - mu[e]) * rs[e]) * gm[e] + bt[e];
                a[e] = (half_t)(f > 0.f ? f : 0.f);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (q == 0) { best[e] = a[e]; id[e] = 0; }
            else if ((float)a[e] > (float)best[e]) { best[e] = a[e]; id[e] = q; }
        }
    }
    *(half8*)(pool + (((int64_t)img * (hp + 2) + py + 1) * (wp + 2) + px + 1) * 64 + c0) = best;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { lo |= id[e] << (8 * e); hi |= id[4 + e] << (8 * e); }
    *(uint2*)(idx + m * 64 + c0) = make_uint2(lo, hi);
}

// m = dpool (pool > 0) at pooled resolution in st_reduce_kernel's row order: part[g][0][c] = sum m, part[g][1][c] = sum m xh at the conv
// position the element's idx byte names, xh = (z - mu) rstd gathered from z; pmax[g][c] = max |m|.  A live element's byte is an in-image
// position by the forward's rule; where the pooled value is 0 the byte is unspecified: it adds nothing and is not decoded.  The decoded
// position is checked against the conv map all the same, so no byte can make an address outside z
__global__ __launch_bounds__(ST_THREADS) void sb_reduce_kernel(const float* dpool, const half_t* pool, const uint8_t* idx, const float* z, const float* tab,
                                                               int64_t rows, int64_t per, int hc, int wc, int hp, int wp, double* part, float* pmax) {
    const int t = threadIdx.x, c = t & 63, k = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t r = m1 - m0, lo = m0 + (k * r + 3) / 4, hi = m0 + ((k + 1) * r + 3) / 4;
    const int HW = hp * wp;
    const float mu = tab[c], rs = tab[64 + c];
    double s1 = 0.0, s2 = 0.0;
    float mx = 0.f;
    if (lo < hi) {
        int img = (int)(lo / HW), rem = (int)(lo - (int64_t)img * HW), y = rem / wp, x = rem - y * wp;
        for (int64_t m = lo; m < hi; ++m) {
            const bool live = (float)pool[(((int64_t)img * (hp + 2) + y + 1) * (wp + 2) + x + 1) * 64 + c] > 0.f;
            if (live) {
                const float a = dpool[m * 64 + c];
                const int code = idx[m * 64 + c], cy = 2 * y - 1 + code / 3, cx = 2 * x - 1 + code % 3;
                s1 += (double)a;
                mx = st_nmax(mx, fabsf(a));
                if (code < 9 && cy >= 0 && cy < hc && cx >= 0 && cx < wc) {
                    const float xh = (z[(((int64_t)img * hc + cy) * wc + cx) * 64 + c] - mu) * rs;
                    s2 += (double)a * (double)xh;
                }
            }
            if (++x == wp) { x = 0; if (++y == hp) { y = 0; ++img; } }
        }
    }
    __shared__ double sh1[ST_THREADS], sh2[ST_THREADS];
    __shared__ float shm[ST_THREADS];
    sh1[t] = s1; sh2[t] = s2; shm[t] = mx;
    __syncthreads();
    if (k == 0) {
        part[(int64_t)blockIdx.x * 128 + c] = (sh1[c] + sh1[64 + c]) + (sh1[128 + c] + sh1[192 + c]);
        part[(int64_t)blockIdx.x * 128 + 64 + c] = (sh2[c] + sh2[64 + c]) + (sh2[128 + c] + sh2[192 + c]);
        pmax[(int64_t)blockIdx.x * 64 + c] = st_nmax(st_nmax(shm[c], shm[64 + c]), st_nmax(shm[128 + c], shm[192 + c]));
    }
}

// One workgroup of 64 threads, thread c = channel c.  The partials in workgroup order (fp64).  dbeta = s1, dgamma = s2 with the incoming
// scale undone; coef = {gamma rstd, s1 / M, s2 / M} [3][64] at the incoming scale, M the conv rows; out_sc = {total scale, 1 / total, this
// stage's multiplier, 0}: a power of two from the bound max_c |gamma rstd| (4 max |m| + |s1| / M + max |xh| |s2| / M) >= max |dz| -- up to
// four windows add into one conv position -- (1 when that is zero or not finite)
__global__ __launch_bounds__(64) void sb_finish_kernel(const double* part, const float* pmax, int G, double inv_m, const float* tab, const float* in_sc,
                                                       float* coef, float* dgam, float* dbet, float* out_sc) {
    const int c = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    float mg = 0.f;
#pragma unroll 8
    for (int g = 0; g < G; ++g) {
        s1 += part[(int64_t)g * 128 + c]; s2 += part[(int64_t)g * 128 + 64 + c];
        mg = st_nmax(mg, pmax[(int64_t)g * 64 + c]);
    }
    const float A = tab[128 + c] * tab[64 + c], B = (float)(s1 * inv_m), C = (float)(s2 * inv_m), mx = tab[256 + c];
    coef[c] = A; coef[64 + c] = B; coef[128 + c] = C;
    dbet[c] = (float)(s1 * (double)in_sc[1]);
    dgam[c] = (float)(s2 * (double)in_sc[1]);
    __shared__ float sh[64];
    sh[c] = (float)(fabs((double)A) * (4.0 * (double)mg + fabs((double)B) + (double)mx * fabs((double)C)));
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (c < o) sh[c] = st_nmax(sh[c], sh[c + o]);
        __syncthreads();
    }
    if (c == 0) {
        const float bound = sh[0];
        const double tin = (double)in_sc[0];
        int e = 0;
        if (bound > 0.f && isfinite(bound)) e = (int)floor(log2((double)SB_SCALE_TARGET / (double)bound));
        const int ein = (tin > 0.0 && isfinite(tin)) ? ilogb(tin) : 0;
        int et = ein + e;
        et = et < -120 ? -120 : et > 120 ? 120 : et;
        e = et - ein;
        const double tot = tin * ldexp(1.0, e);
        out_sc[0] = (float)tot; out_sc[1] = (float)(1.0 / tot); out_sc[2] = ldexpf(1.0f, e); out_sc[3] = 0.f;
    }
}

// dZ[row][c] = gamma rstd (g - s1 / M - xh s2 / M) in fp32, times the multiplier, as fp16, for conv pixel row = (img, y, x): g is m gathered
// by st_form_kernel's membership rule, the 1, 2 or 4 windows that hold the pixel and whose idx names it, added in (py, px) order; xh from
// the saved z.  Nothing is scattered.  One thread = 8 channels of one conv pixel.
__global__ __launch_bounds__(ST_THREADS) void sb_form_kernel(const float* dpool, const half_t* pool, const uint8_t* idx, const float* z, const float* tab,
                                                             const float* coef, const float* sc, int64_t rows, int hc, int wc, int hp, int wp, half_t* dz) {
    const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= rows * 8) return;
    const int c0 = (int)(i & 7) * 8;
    const int64_t m = i >> 3;
    const int HW = hc * wc, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / wc, x = rem - y * wc;
    const float mul = sc[2];
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int py0 = y >> 1, py1 = (y + 1) >> 1, px0 = x >> 1, px1 = (x + 1) >> 1;
    for (int py = py0; py <= py1 && py < hp; ++py)
        for (int px = px0; px <= px1 && px < wp; ++px) {
            const int code = 3 * (y - 2 * py + 1) + (x - 2 * px + 1);
            const int64_t pp = ((int64_t)img * hp + py) * wp + px;
            const uint2 ib = *(const uint2*)(idx + pp * 64 + c0);
            const half8 pv = *(const half8*)(pool + (((int64_t)img * (hp + 2) + py + 1) * (wp + 2) + px + 1) * 64 + c0);
            const floatx4 d0 = *(const floatx4*)(dpool + pp * 64 + c0), d1 = *(const floatx4*)(dpool + pp * 64 + c0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if ((int)((ib.x >> (8 * e)) & 0xff) == code && (float)pv[e] > 0.f) acc[e] += d0[e];
                if ((int)((ib.y >> (8 * e)) & 0xff) == code && (float)pv[4 + e] > 0.f) acc[4 + e] += d1[e];
            }
        }
    half8 h;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const floatx4 zv = *(const floatx4*)(z + i * 8 + 4 * k);
        const floatx4 mu = *(const floatx4*)(tab + c0 + 4 * k), rs = *(const floatx4*)(tab + 64 + c0 + 4 * k);
        const floatx4 A = *(const floatx4*)(coef + c0 + 4 * k), B = *(const floatx4*)(coef + 64 + c0 + 4 * k), C = *(const floatx4*)(coef + 128 + c0 + 4 * k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (zv[e] - mu[e]) * rs[e];
            h[4 * k + e] = (half_t)(A[e] * (acc[4 * k + e] - B[e] - xh * C[e]) * mul);
        }
    }
    *(half8*)(dz + i * 8) = h;
}

// One workgroup per output channel c, thread k < 147 = (ci, ky, kx) in the weight's own order: dW = the slabs summed in slab order (fp64)
// with the scale undone, read at column 32 ky + 4 kx + ci.  dz carries gamma rstd: no factor follows
__global__ __launch_bounds__(ST_THREADS) void sb_dw_kernel(const float* slab, int S, const float* sc, float* dw) {
    const int c = blockIdx.x, t = threadIdx.x;
    if (t >= 147) return;
    const int ci = t / 49, ky = (t % 49) / 7, kx = t % 7, q = 32 * ky + 4 * kx + ci;
    double G = 0.0;
    for (int s = 0; s < S; ++s) G += (double)slab[((int64_t)s * SW_P + c) * SW_Q + q];
    dw[c * 147 + t] = (float)(G * (double)sc[1]);
}

bool params_ok(const vtd_stem_params* p) {
    return p && p->w && p->gamma && p->beta && p->mean && p->var &&
           !(((uintptr_t)p->w | (uintptr_t)p->gamma | (uintptr_t)p->beta | (uintptr_t)p->mean | (uintptr_t)p->var) & 3);
}

}  // namespace

int vtd_launch_stem_pack_input(const void* x, int dtype, int n, int H, int W, void* tap, hipStream_t s) {
    Geo g;
    if (!x || !tap || !make_geo(n, H, W, g) || dtype < 0 || dtype > 1) return ST_ARG;
    if (((uintptr_t)x & (dtype ? 1 : 3)) || ((uintptr_t)tap & 15)) return ST_ALIGN;
    const unsigned blocks = nblk((int64_t)n * (H + 6) * (W + 6));
    if (dtype)
        hipLaunchKernelGGL(st_pack_kernel<half_t>, dim3(blocks), dim3(ST_THREADS), 0, s, (const half_t*)x, n, H, W, (half_t*)tap);
    else
        hipLaunchKernelGGL(st_pack_kernel<float>, dim3(blocks), dim3(ST_THREADS), 0, s, (const float*)x, n, H, W, (half_t*)tap);
    return -(int)hipGetLastError();
}

int64_t vtd_stem_ws_bytes(int n, int H, int W, int mode) {
    Geo g;
    if (!make_geo(n, H, W, g) || mode < 0 || mode > 1) return ST_ARG;
    return mode ? bwd_layout(g).total : fwd_layout().total;
}

int vtd_launch_stem_forward(const void* x, int n, int H, int W, const vtd_stem_params* P, float eps, void* ws, void* pool, void* idx, hipStream_t s) {
    Geo g;
    if (!x || !ws || !pool || !idx || !make_geo(n, H, W, g) || !params_ok(P) || !(eps > 0.f)) return ST_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)pool & 15) || ((uintptr_t)idx & 7) || ((uintptr_t)ws & 255)) return ST_ALIGN;
    const FwdLayout L = fwd_layout();
    half_t* wfrag = (half_t*)((char*)ws + L.w);
    float* bias = (float*)((char*)ws + L.bias);
    hipLaunchKernelGGL(st_fold_kernel, dim3(nblk(ST_WFRAG + 64)), dim3(ST_THREADS), 0, s, (const float*)P->w, (const float*)P->gamma, (const float*)P->beta,
                       (const float*)P->mean, (const float*)P->var, eps, wfrag, bias);
    hipLaunchKernelGGL(st_zero_ring_kernel, dim3(nblk((int64_t)n * (2 * (g.wp + 2) + 2 * g.hp) * 8)), dim3(ST_THREADS), 0, s, (half_t*)pool, n, g.hp, g.wp);
    StemFwdParams p;
    p.in = (const half_t*)x; p.w = wfrag; p.bias = bias; p.out = (half_t*)pool; p.idx = (uint8_t*)idx; p.z = nullptr;
    p.n = n; p.in_hp = H + 6; p.in_wp = W + 6; p.conv_h = g.hc; p.conv_w = g.wc; p.pool_h = g.hp; p.pool_w = g.wp;
    p.tiles_x = (g.wp + ST_PT_COLS - 1) / ST_PT_COLS;
    p.tiles_y = (g.hp + ST_PT_ROWS - 1) / ST_PT_ROWS;
    const int64_t tiles = (int64_t)n * p.tiles_x * p.tiles_y;
    if (tiles >= (1ll << 31)) return ST_ARG;
    hipLaunchKernelGGL(stem_train_forward_kernel<false>, dim3((unsigned)tiles), dim3(ST_THREADS), 0, s, p);
    return -(int)hipGetLastError();
}

int vtd_launch_stem_backward(const void* x, int n, int H, int W, const vtd_stem_params* P, float eps, const void* ws, const void* pool, const void* idx,
                             const float* dpool, const float* dscale, const vtd_stem_params* Gp, void* scratch, hipStream_t s) {
    Geo g;
    if (!x || !ws || !pool || !idx || !dpool || !dscale || !scratch || !make_geo(n, H, W, g) || !params_ok(P) || !Gp || !Gp->w || !Gp->gamma || !Gp->beta ||
        !(eps > 0.f))
        return ST_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)pool & 15) || ((uintptr_t)idx & 7) || ((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255) || ((uintptr_t)dpool & 15) ||
        ((uintptr_t)dscale & 7) || (((uintptr_t)Gp->w | (uintptr_t)Gp->gamma | (uintptr_t)Gp->beta) & 3))
        return ST_ALIGN;
    const BwdLayout B = bwd_layout(g);
    char* q = (char*)scratch;
    half_t* dz = (half_t*)(q + B.dz);
    double *part = (double*)(q + B.part), *sum = (double*)(q + B.sum);
    float *pmax = (float*)(q + B.pmax), *sc = (float*)(q + B.sc), *slab = (float*)(q + B.slab);
    int Gr = (int)((g.mp + 255) / 256);
    Gr = Gr < 1 ? 1 : Gr > ST_MAX_RED ? ST_MAX_RED : Gr;
    const int64_t per = (g.mp + Gr - 1) / Gr;
    hipLaunchKernelGGL(st_reduce_kernel, dim3(Gr), dim3(ST_THREADS), 0, s, dpool, (const half_t*)pool, g.mp, per, g.hp, g.wp, part, pmax);
    hipLaunchKernelGGL(st_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)part, (const float*)pmax, Gr, dscale, sum, sc);
    hipLaunchKernelGGL(st_form_kernel, dim3(nblk(g.mc * 8)), dim3(ST_THREADS), 0, s, dpool, (const half_t*)pool, (const uint8_t*)idx, (const float*)sc, g.mc,
                       g.hc, g.wc, g.hp, g.wp, dz);
    VTD_HIP_CHECK(hipGetLastError());
    const int S = wg_slabs(g.mc);
    StemWgArgs wa;
    wa.dz = dz; wa.x = (const half_t*)x; wa.hc = g.hc; wa.wc = g.wc; wa.in_hp = H + 6; wa.in_wp = W + 6; wa.rows = g.mc; wa.slab_len = slab_rows(g.mc, S);
    wa.slab = slab;
    hipLaunchKernelGGL(stem_train_wgrad_kernel, dim3(S), dim3(ST_THREADS), 0, s, wa);
    hipLaunchKernelGGL(st_param_kernel, dim3(64), dim3(ST_THREADS), 0, s, (const float*)slab, S, (const float*)sc, (const double*)sum, (const float*)P->w,
                       (const float*)P->gamma, (const float*)P->mean, (const float*)P->var, eps, Gp->w, Gp->gamma, Gp->beta);
    return -(int)hipGetLastError();
}

// ---- the batch-statistics entries: training = 0 is the frozen path above, its bits ----------------------------------------------------------
int64_t vtd_stem_bn_ws_bytes(int n, int H, int W, int mode) {
    Geo g;
    if (!make_geo(n, H, W, g) || mode < 0 || mode > 1) return SB_ARG;
    // either value of `training` runs in one allocation: the frozen layout starts at offset 0 too
    const int64_t frozen = mode ? bwd_layout(g).total : fwd_layout().total, own = mode ? bn_bwd_layout(g).total : bn_fwd_layout(g).total;
    return frozen > own ? frozen : own;
}

int vtd_launch_stem_bn_forward(const void* x, int n, int H, int W, const vtd_stem_params* P, int training, float momentum, float eps, void* ws, void* pool,
                               void* idx, float* stats, hipStream_t s) {
    Geo g;
    if (!x || !ws || !pool || !idx || !make_geo(n, H, W, g) || !params_ok(P) || !(eps > 0.f) || (training != 0 && training != 1)) return SB_ARG;
    if (training && (g.mc < 2 || !(momentum >= 0.f && momentum <= 1.f))) return SB_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)pool & 15) || ((uintptr_t)idx & 7) || ((uintptr_t)ws & 255) || ((uintptr_t)stats & 3)) return SB_ALIGN;
    if (!training) return vtd_launch_stem_forward(x, n, H, W, P, eps, ws, pool, idx, s);
    const BnFwdLayout L = bn_fwd_layout(g);
    char* w = (char*)ws;
    half_t* wfrag = (half_t*)(w + L.w);
    float *tab = (float*)(w + L.tab), *pmm = (float*)(w + L.pmm), *z = (float*)(w + L.z);
    double* part = (double*)(w + L.part);
    hipLaunchKernelGGL(sb_pack_kernel, dim3(nblk(ST_WFRAG)), dim3(ST_THREADS), 0, s, (const float*)P->w, wfrag);
    hipLaunchKernelGGL(st_zero_ring_kernel, dim3(nblk((int64_t)n * (2 * (g.wp + 2) + 2 * g.hp) * 8)), dim3(ST_THREADS), 0, s, (half_t*)pool, n, g.hp, g.wp);
    StemFwdParams p;
    p.in = (const half_t*)x; p.w = wfrag; p.bias = nullptr; p.out = nullptr; p.idx = nullptr; p.z = z;
    p.n = n; p.in_hp = H + 6; p.in_wp = W + 6; p.conv_h = g.hc; p.conv_w = g.wc; p.pool_h = g.hp; p.pool_w = g.wp;
    p.tiles_x = (g.wp + ST_PT_COLS - 1) / ST_PT_COLS;
    p.tiles_y = (g.hp + ST_PT_ROWS - 1) / ST_PT_ROWS;
    const int64_t tiles = (int64_t)n * p.tiles_x * p.tiles_y;
    if (tiles >= (1ll << 31)) return SB_ARG;
    hipLaunchKernelGGL(stem_train_forward_kernel<true>, dim3((unsigned)tiles), dim3(ST_THREADS), 0, s, p);
    VTD_HIP_CHECK(hipGetLastError());
    const int Gr = bn_red(g.mc);
    const int64_t per = (g.mc + Gr - 1) / Gr;
    hipLaunchKernelGGL(sb_stats_partial_kernel, dim3(Gr), dim3(ST_THREADS), 0, s, (const float*)z, g.mc, per, part, pmm);
    hipLaunchKernelGGL(sb_stats_finish_kernel, dim3(64), dim3(ST_THREADS), 0, s, (const double*)part, (const float*)pmm, Gr, (const float*)P->gamma, (const float*)P->beta,
                       P->mean, P->var, momentum, eps, tab, stats);
    hipLaunchKernelGGL(sb_pool_kernel, dim3(nblk(g.mp * 8)), dim3(ST_THREADS), 0, s, (const float*)z, (const float*)tab, g.mp, g.hc, g.wc, g.hp, g.wp,
                       (half_t*)pool, (uint8_t*)idx);
    return -(int)hipGetLastError();
}

int vtd_launch_stem_bn_backward(const void* x, int n, int H, int W, const vtd_stem_params* P, int training, float eps, const void* ws, const void* pool,
                                const void* idx, const float* dpool, const float* dscale, const vtd_stem_params* Gp, void* scratch, hipStream_t s) {
    Geo g;
    if (!x || !ws || !pool || !idx || !dpool || !dscale || !scratch || !make_geo(n, H, W, g) || !params_ok(P) || !Gp || !Gp->w || !Gp->gamma || !Gp->beta ||
        !(eps > 0.f) || (training != 0 && training != 1) || (training && g.mc < 2))
        return SB_ARG;
    if (((uintptr_t)x & 15) || ((uintptr_t)pool & 15) || ((uintptr_t)idx & 7) || ((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255) || ((uintptr_t)dpool & 15) ||
        ((uintptr_t)dscale & 7) || (((uintptr_t)Gp->w | (uintptr_t)Gp->gamma | (uintptr_t)Gp->beta) & 3))
        return SB_ALIGN;
    if (!training) return vtd_launch_stem_backward(x, n, H, W, P, eps, ws, pool, idx, dpool, dscale, Gp, scratch, s);
    const BnFwdLayout L = bn_fwd_layout(g);
    const BnBwdLayout B = bn_bwd_layout(g);
    const char* w = (const char*)ws;
    char* q = (char*)scratch;
    const float *z = (const float*)(w + L.z), *tab = (const float*)(w + L.tab);
    half_t* dz = (half_t*)(q + B.dz);
    double* part = (double*)(q + B.part);
    float *pmax = (float*)(q + B.pmax), *coef = (float*)(q + B.coef), *sc = (float*)(q + B.sc), *slab = (float*)(q + B.slab);
    int Gr = (int)((g.mp + 255) / 256);      // st_reduce_kernel's rows: the pooled pixels
    Gr = Gr < 1 ? 1 : Gr > ST_MAX_RED ? ST_MAX_RED : Gr;
    const int64_t per = (g.mp + Gr - 1) / Gr;
    hipLaunchKernelGGL(sb_reduce_kernel, dim3(Gr), dim3(ST_THREADS), 0, s, dpool, (const half_t*)pool, (const uint8_t*)idx, z, tab, g.mp, per, g.hc, g.wc, g.hp,
                       g.wp, part, pmax);
    hipLaunchKernelGGL(sb_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)part, (const float*)pmax, Gr, 1.0 / (double)g.mc, tab, dscale, coef, Gp->gamma,
                       Gp->beta, sc);
    hipLaunchKernelGGL(sb_form_kernel, dim3(nblk(g.mc * 8)), dim3(ST_THREADS), 0, s, dpool, (const half_t*)pool, (const uint8_t*)idx, z, tab, (const float*)coef,
                       (const float*)sc, g.mc, g.hc, g.wc, g.hp, g.wp, dz);
    VTD_HIP_CHECK(hipGetLastError());
    const int S = wg_slabs(g.mc);
    StemWgArgs wa;
    wa.dz = dz; wa.x = (const half_t*)x; wa.hc = g.hc; wa.wc = g.wc; wa.in_hp = H + 6; wa.in_wp = W + 6; wa.rows = g.mc; wa.slab_len = slab_rows(g.mc, S);
    wa.slab = slab;
    hipLaunchKernelGGL(stem_train_wgrad_kernel, dim3(S), dim3(ST_THREADS), 0, s, wa);
    hipLaunchKernelGGL(sb_dw_kernel, dim3(64), dim3(ST_THREADS), 0, s, (const float*)slab, S, (const float*)sc, Gp->w);
    return -(int)hipGetLastError();
}
