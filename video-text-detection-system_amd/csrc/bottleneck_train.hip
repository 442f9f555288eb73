// ResNet Bottleneck (v1.5: the stride sits on the 3x3) training with frozen-statistics BatchNorm (the running statistics normalise and are
// never written; gamma and beta learn), forward and backward, for the blocks of ResNet-50's four stages.  One host path and one set of
// kernels serve every width W; each stage has its own C entries and error codes:
//   res5 (torchvision's layer4), W = 512: (1024 -> 512 -> 2048, stride 2, downsample) and (2048 -> 512 -> 2048, stride 1, identity)
//   res4 (torchvision's layer3), W = 256: (512 -> 256 -> 1024, stride 2, downsample) and (1024 -> 256 -> 1024, stride 1, identity)
//   res3 (torchvision's layer2), W = 128: (256 -> 128 -> 512, stride 2, downsample) and (512 -> 128 -> 512, stride 1, identity)
//   res2 (torchvision's layer1), W = 64: (64 -> 64 -> 256, stride 1, downsample at stride 1) and (256 -> 64 -> 256, stride 1, identity)
// Tensors are padded taps (ring-padded NHWC fp16, ring 1).  y = relu(bn3(conv3(a2)) + id), a2 = relu(bn2(conv2(a1))), a1 = relu(bn1(conv1(x))),
// id = x or ds_bn(ds(x)); conv1 1x1 cin -> W, conv2 3x3 at stride s, conv3 1x1 W -> 4 W, ds 1x1 cin = 2 W (res2: W) -> 4 W at stride s.
//
// Forward:
//   fold             per convolution (rb_fold_kernel): w gamma rstd -> fp16 GEMM panel [cout][ksz^2 cin] (k = tap * cin + ci), bias = beta -
//                    mean gamma rstd; on the device, every call
//   conv x 3 or 4    conv_igemm.hip: conv1 (ReLU) -> padded a1 at the INPUT's extent; conv2 (stride s, ReLU) -> padded a2; downsample
//                    (the block's stride) -> padded id; conv3 (EPI_RESIDUAL from id or x, ReLU) -> padded y.  a1, a2 and id stay in the workspace
// Backward from dy (NHWC fp32 [n h w][4 W] times a power of two):
//   mask + reduce    bk_mask_reduce_kernel<4 W / 1024>, one pass over the 4 W-wide gradient: g3 = dy (y > 0) in fp32 (the gradient at bn3's
//                    output, of the downsample's BatchNorm output, and of an identity input) with its per-channel fp64 partial sums and
//                    max |.|.  G = min(256, ceil(rows / 32)) workgroups of ceil(rows / G) consecutive rows each, in row order; thread t
//                    owns channels 1024 j + 4 t .. 1024 j + 4 t + 3 (j < 2 at W = 512, j = 0 at W = 256), so every wave load is 1 KiB of
//                    one row and a workgroup's loads are the whole row.  rb_finish_kernel adds the partials in workgroup order and gives
//                    the power-of-two scale.  W = 128 (4 W = 512 < 1024): bk_mask_reduce512_kernel, the same grid and contract; threads
//                    0 .. 127 own the row's 512 channels (4 each) over the first ceil(r / 2) of the workgroup's r rows and threads
//                    128 .. 255 over the rest, so a wave load is still 1 KiB of one row; part = first half + second half (through LDS).
//                    W = 64 (4 W = 256): bk_mask_reduce256_kernel, the same again in four row quarters of 64 threads each, split as
//                    rb_reduce64_kernel splits them (15 rows -> 4, 4, 4, 3); part = (q0 + q1) + (q2 + q3)
//   form             rb_form_kernel: the fp16 operands, flat [rows][C] for the weight gradients and ring-padded for the transposed convolutions
//   g2, g1           the W-wide stages as resblock_train.hip's: rb_mask_kernel, rb_reduce_kernel (min(256, ceil(rows / 256)) workgroups; one
//                    channel per thread at W = 256, two at 512; W = 128: rb_reduce128_kernel, two row halves per workgroup; W = 64:
//                    rb_reduce64_kernel, four row quarters), finish, form.
//                    g1 lives at the input's extent (conv1 is 1x1 at stride 1 in front of the strided 3x3)
//   wgrad<3>         G[c][k] = sum_m g[m][c] x[m][k] on wgrad_mfma.h as it stands: conv3 (lda 4 W: 4 W / 128 column tiles, xc W, 1x1), conv2
//                    (lda W, xc W, 3x3 at stride s over a1), conv1 (lda W, xc = cin, 1x1, rows = n h_in w_in) and the downsample
//                    (lda 4 W, xc 2 W, 1x1 at stride 2).  Slabs: min(8, ceil(rows / 4096)) of the LAUNCH's rows -- conv1's are the
//                    input's, the others' the output's.  res3 only (W = 128, where that rule leaves 2 .. 32 workgroups for 256 CUs):
//                    wg_slabs_tiles, slabs = min(ceil(512 / (q-tiles x column tiles)), ceil(rows / 1024)) -- 512 workgroups when the rows
//                    allow slabs of 1024 rows; shape-only.  res2 (W = 64) takes the same rule on the other two modes of wgrad_mfma.h:
//                    conv2 and conv1 (lda 64) on MODE 5, the 64-row tile with one column tile, slab [64][ksz^2 xc] (conv2: K = 576, 5
//                    q-tiles; conv1: xc = 256 or 64, 2 or 1); conv3 and the downsample (lda 256, xc 64, 1x1) on MODE 4, two column
//                    tiles and half a q-tile.  rb_param_kernel's grid is lda, so its slab stride is the launch's either way
//   param            rb_param_kernel: slabs summed in order in fp64; dW = gamma rstd G, dbeta = s, dgamma = rstd (sum_k w G - mean s)
//   da2              conv3^T(g3): a 1x1 GEMM 4 W -> W on the transposed folded weights (conv_igemm.hip, fp32 output); g2 = da2 (a2 > 0)
//   da1              conv2^T(g2): the folded weights rotated by 180 degrees and transposed, 3x3 at stride 1.  Stride 2: g2 is written to
//                    the even positions of a zeroed ring-padded plane of the input's extent first (Z[2o][2p] = g2[o][p]), then the same
//                    path -- the form resblock_train.hip documents.  g1 = da1 (a1 > 0)
//   dx (optional)    conv1^T(g1), a 1x1 GEMM W -> cin at g1's total scale; plus, stride 1, g3 times the product of the three stages'
//                    power-of-two multipliers; or, stride 2, ds^T(g3) (a 1x1 GEMM 4 W -> 2 W at g3's scale) times the product of the
//                    two lower stages' multipliers at the even (row, column) positions; or, res2.0 (downsample at stride 1), the same
//                    ds^T(g3) (4 W -> W) times the same product at every pixel (rb_add_identity_kernel's dense sum)
// No atomics, shape-only grids, fixed summation orders: bitwise repeatable.
#include "resblock_common.h"

#include "conv_kernels.h"

namespace {

constexpr int BK_MAX_RED = 256;

// an entry family: the Bottleneck width it accepts and its error-code pair
struct Fam { int width, err_arg, err_align; };
constexpr Fam BK_RES5 = {512, -3901, -3902}, BK_RES4 = {256, -3903, -3904}, BK_RES3 = {128, -3905, -3906}, BK_RES2 = {64, -3907, -3908};

struct Geo {
    int n, hin, win, cin, stride, h, w;
    int W, OUT;                  // the Bottleneck width and 4 W
    int64_t m, min, pin, pout;   // output rows, input rows, padded pixels of the input's and the output's extent
    bool ds;                     // the block has a downsample (1x1 at the block's stride): a stage's first block
};

bool make_geo(const Fam& fam, int n, int hin, int win, int cin, int width, int stride, Geo& g) {
    const int W = fam.width, OUT = 4 * W;
    if (n <= 0 || hin <= 0 || win <= 0 || n > 65535 || hin > 4096 || win > 4096 || width != W) return false;
    // a stage's first block: res3 .. res5 halve the extent from 2 W channels; res2 (W = 64) follows the max-pool at stride 1 from W channels
    const bool first = W == 64 ? cin == W && stride == 1 : cin == 2 * W && stride == 2 && !(hin & 1) && !(win & 1);
    if (!(first || (cin == OUT && stride == 1))) return false;
    g.W = W; g.OUT = OUT;
    g.n = n; g.hin = hin; g.win = win; g.cin = cin; g.stride = stride; g.h = hin / stride; g.w = win / stride;
    g.m = (int64_t)n * g.h * g.w; g.min = (int64_t)n * hin * win;
    g.pin = (int64_t)n * (hin + 2) * (win + 2); g.pout = (int64_t)n * (g.h + 2) * (g.w + 2);
    g.ds = first;
    // every tensor the convolutions index: x, a1 and the planes of the input's extent, y and id
    return g.pin * (cin > W ? cin : W) < (1ll << 31) && g.pout * OUT < (1ll << 31);
}

// the slabs of a weight-gradient launch over `rows` rows with `nqt` q-tiles and lda / 128 column tiles (one for the 64-row tile of a 64-wide
// gradient): res5 and res4 by the rows alone, res3 and res2 (W <= 128) by the workgroups the launch would otherwise lack
int bk_slabs(const Geo& g, int64_t rows, int nqt, int lda) {
    return g.W <= 128 ? wg_slabs_tiles(rows, nqt, lda < 128 ? 1 : lda / 128) : wg_slabs(rows);
}

struct FwdLayout { int64_t a1, a2, id, w1, w2, w3, wd, bias, total; };
struct BwdLayout { int64_t g3, g2, g1, g3h, g2h, g1h, g3p, g2p, g1p, wt, zero, part, pmax, sum3, sum2, sum1, sc, slab, total; };

FwdLayout fwd_layout(const Geo& g) {
    FwdLayout L;
    const int W = g.W, OUT = g.OUT;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    L.a1 = take(g.pin * W * 2); L.a2 = take(g.pout * W * 2); L.id = take(g.ds ? g.pout * OUT * 2 : 0);
    L.w1 = take((int64_t)W * g.cin * 2); L.w2 = take((int64_t)W * 9 * W * 2); L.w3 = take((int64_t)OUT * W * 2);
    L.wd = take(g.ds ? (int64_t)OUT * g.cin * 2 : 0);
    L.bias = take((2 * W + 2 * OUT) * 4);
    L.total = o;
    return L;
}

BwdLayout bwd_layout(const Geo& g) {
    BwdLayout L;
    const int W = g.W, OUT = g.OUT;
    int64_t o = 0;
    auto take = [&](int64_t b) { const int64_t r = o; o += a256(b); return r; };
    L.g3 = take(g.m * OUT * 4); L.g2 = take(g.m * W * 4); L.g1 = take(g.min * W * 4);
    L.g3h = take(g.m * OUT * 2); L.g2h = take(g.m * W * 2); L.g1h = take(g.min * W * 2);
    L.g3p = take(g.pout * OUT * 2);
    L.g2p = take(g.pin * W * 2);   // stride 1: g2 ring-padded; stride 2: the zero-inserted plane.  Both of the input's extent
    L.g1p = take(g.pin * W * 2);
    L.wt = take((int64_t)W * 9 * W * 2);   // the largest transposed panel: conv2's 9 W^2 (the downsample's is 2 W x 4 W)
    L.zero = take(OUT * 4);
    L.part = take((int64_t)BK_MAX_RED * OUT * 8); L.pmax = take(BK_MAX_RED * 4);
    L.sum3 = take(OUT * 8); L.sum2 = take(W * 8); L.sum1 = take(W * 8);
    L.sc = take(3 * 4 * 4);
    // conv2's slab [W][9 W] is the largest of the launches over the output's rows (conv3 [4 W][W], the downsample [4 W][2 W]);
    // conv1's [W][cin] goes with the input's rows
    int64_t so = (int64_t)wg_slabs(g.m) * W * 9 * W, si = (int64_t)wg_slabs(g.min) * W * g.cin;
    if (W <= 128) {   // per launch: conv2 and conv1, then conv3 and the downsample
        so = (int64_t)bk_slabs(g, g.m, wg_nqt(3, W), W) * W * 9 * W;
        si = (int64_t)bk_slabs(g, g.min, wg_nqt(1, g.cin), W) * W * g.cin;
        const int64_t s3 = (int64_t)bk_slabs(g, g.m, wg_nqt(1, W), OUT) * OUT * W,
                      sd = g.ds ? (int64_t)bk_slabs(g, g.m, wg_nqt(1, g.cin), OUT) * OUT * g.cin : 0;
        so = s3 > so ? s3 : so;
        so = sd > so ? sd : so;
    }
    L.slab = take((so > si ? so : si) * 4);
    L.total = o;
    return L;
}

// v [rows][OUT] fp32, OUT = 1024 NJ (NJ = 2: res5's 2048-wide gradient, NJ = 1: res4's 1024-wide one), act the ring-padded fp16 activation
// [n][H + 2][Wd + 2][OUT]: out = v where act > 0, else 0 (in place when out == v), and over the workgroup's rows m0 .. m1 - 1 in row order
// the per-channel fp64 sums of out: part[g][OUT], pmax[g] = max |out| (NaN kept).
// Thread t owns channels 1024 j + 4 t .. 1024 j + 4 t + 3 for j < NJ: a wave's 16-byte loads cover 1 KiB of the row.
template <int NJ>
__global__ __launch_bounds__(RB_THREADS) void bk_mask_reduce_kernel(const float* v, const half_t* act, int64_t rows, int64_t per, int H, int Wd, float* out,
                                                                    double* part, float* pmax) {
    const int t = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    constexpr int OUT = 1024 * NJ;
    double s[4 * NJ];
#pragma unroll
    for (int k = 0; k < 4 * NJ; ++k) s[k] = 0.0;
    float mx = 0.f;
    const int HW = H * Wd;
    int img = (int)(m0 / HW), rem = (int)(m0 - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    for (int64_t m = m0; m < m1; ++m) {
        const half_t* a = act + (((int64_t)img * (H + 2) + y + 1) * (Wd + 2) + x + 1) * OUT;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = j * 1024 + 4 * t;
            const floatx4 f = *(const floatx4*)(v + m * OUT + c);
            const half4 hh = *(const half4*)(a + c);
            floatx4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = (float)hh[e] > 0.f ? f[e] : 0.f;
                s[4 * j + e] += (double)o[e];
                const float fa = fabsf(o[e]);
                mx = fa > mx || fa != fa ? fa : mx;
            }
            *(floatx4*)(out + m * OUT + c) = o;
        }
        if (++x == Wd) { x = 0; if (++y == H) { y = 0; ++img; } }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[(int64_t)blockIdx.x * OUT + j * 1024 + 4 * t + e] = s[4 * j + e];
    __shared__ float shm[RB_THREADS];
    shm[t] = mx;
    __syncthreads();
    if (t == 0) {
        float q = shm[0];
        for (int k = 1; k < RB_THREADS; ++k) q = shm[k] > q || shm[k] != shm[k] ? shm[k] : q;
        pmax[blockIdx.x] = q;
    }
}

// The 512-wide form (res3, OUT = 512 < 1024): the same contract.  Thread t owns channels 4 (t % 128) .. 4 (t % 128) + 3 over one half of the
// workgroup's rows m0 .. m1 - 1 in row order, t < 128 the first ceil((m1 - m0) / 2) rows and t >= 128 the rest (rb_reduce128_kernel's split), so
// a wave's 16-byte loads are still 1 KiB of one row and the two halves stream two rows at a time; part[g][c] = the first half's sum + the second
// half's (handed over through LDS), fp64; pmax[g] over both halves, NaN kept.
__global__ __launch_bounds__(RB_THREADS) void bk_mask_reduce512_kernel(const float* v, const half_t* act, int64_t rows, int64_t per, int H, int Wd, float* out,
                                                                       double* part, float* pmax) {
    constexpr int OUT = 512;
    const int t = threadIdx.x, c = 4 * (t & 127), hf = t >> 7;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t mid = m0 + (m1 - m0 + 1) / 2, lo = hf ? mid : m0, hi = hf ? m1 : mid;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    float mx = 0.f;
    const int HW = H * Wd;
    int img = (int)(lo / HW), rem = (int)(lo - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    for (int64_t m = lo; m < hi; ++m) {
        const half_t* a = act + (((int64_t)img * (H + 2) + y + 1) * (Wd + 2) + x + 1) * OUT;
        const floatx4 f = *(const floatx4*)(v + m * OUT + c);
        const half4 hh = *(const half4*)(a + c);
        floatx4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = (float)hh[e] > 0.f ? f[e] : 0.f;
            s[e] += (double)o[e];
            const float fa = fabsf(o[e]);
            mx = fa > mx || fa != fa ? fa : mx;
        }
        *(floatx4*)(out + m * OUT + c) = o;
        if (++x == Wd) { x = 0; if (++y == H) { y = 0; ++img; } }
    }
    __shared__ double shs[OUT];
    __shared__ float shm[RB_THREADS];
    if (hf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) shs[c + e] = s[e];
    }
    shm[t] = mx;
    __syncthreads();
    if (!hf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) part[(int64_t)blockIdx.x * OUT + c + e] = s[e] + shs[c + e];
    }
    if (t == 0) {
        float q = shm[0];
        for (int k = 1; k < RB_THREADS; ++k) q = shm[k] > q || shm[k] != shm[k] ? shm[k] : q;
        pmax[blockIdx.x] = q;
    }
}

// The 256-wide form (res2, OUT = 256): the same contract.  Thread t owns channels 4 (t % 64) .. 4 (t % 64) + 3 over one quarter of the
// workgroup's r = m1 - m0 rows in row order: quarter k = t / 64 takes rows m0 + ceil(k r / 4) .. m0 + ceil((k + 1) r / 4) - 1
// (rb_reduce64_kernel's split: 15 rows -> 4, 4, 4, 3), so a wave's 16-byte loads are still 1 KiB of one row and the four quarters stream four
// rows at a time; part[g][c] = (q0 + q1) + (q2 + q3) (handed over through LDS), fp64; pmax[g] over all four, NaN kept.
__global__ __launch_bounds__(RB_THREADS) void bk_mask_reduce256_kernel(const float* v, const half_t* act, int64_t rows, int64_t per, int H, int Wd, float* out,
                                                                       double* part, float* pmax) {
    constexpr int OUT = 256;
    const int t = threadIdx.x, c = 4 * (t & 63), k = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * per < rows ? (int64_t)blockIdx.x * per : rows, m1 = m0 + per < rows ? m0 + per : rows;
    const int64_t r = m1 - m0, lo = m0 + (k * r + 3) / 4, hi = m0 + ((k + 1) * r + 3) / 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    float mx = 0.f;
    const int HW = H * Wd;
    int img = (int)(lo / HW), rem = (int)(lo - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    for (int64_t m = lo; m < hi; ++m) {
        const half_t* a = act + (((int64_t)img * (H + 2) + y + 1) * (Wd + 2) + x + 1) * OUT;
        const floatx4 f = *(const floatx4*)(v + m * OUT + c);
        const half4 hh = *(const half4*)(a + c);
        floatx4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = (float)hh[e] > 0.f ? f[e] : 0.f;
            s[e] += (double)o[e];
            const float fa = fabsf(o[e]);
            mx = fa > mx || fa != fa ? fa : mx;
        }
        *(floatx4*)(out + m * OUT + c) = o;
        if (++x == Wd) { x = 0; if (++y == H) { y = 0; ++img; } }
    }
    __shared__ double shs[4][OUT];
    __shared__ float shm[RB_THREADS];
#pragma unroll
    for (int e = 0; e < 4; ++e) shs[k][c + e] = s[e];
    shm[t] = mx;
    __syncthreads();
    if (k == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) part[(int64_t)blockIdx.x * OUT + c + e] = (shs[0][c + e] + shs[1][c + e]) + (shs[2][c + e] + shs[3][c + e]);
    }
    if (t == 0) {
        float q = shm[0];
        for (int j = 1; j < RB_THREADS; ++j) q = shm[j] > q || shm[j] != shm[j] ? shm[j] : q;
        pmax[blockIdx.x] = q;
    }
}

// stride 1: dx [items4 x 4] (at g1's total scale) += g3 (at the incoming scale) times the three stages' multipliers, powers of two
__global__ __launch_bounds__(RB_THREADS) void bk_add_identity_kernel(float* dx, const float* g3, int64_t items4, const float* sc3, const float* sc2,
                                                                     const float* sc1) {
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    if (i >= items4) return;
    const float mul = sc3[2] * sc2[2] * sc1[2];
    floatx4 a = *(floatx4*)(dx + i * 4);
    const floatx4 b = *(const floatx4*)(g3 + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += b[e] * mul;
    *(floatx4*)(dx + i * 4) = a;
}

// stride 2: dx [n][2H][2Wd][cin] (at g1's total scale) += ds^T(g3) [n][H][Wd][cin] (at g3's total scale) times the two lower stages'
// multipliers, powers of two, at the even (row, column) positions: the 1x1 stride-2 convolution reads no other.  One thread = 4 channels.
__global__ __launch_bounds__(RB_THREADS) void bk_add_downsample_kernel(float* dx, const float* t, int64_t rows, int H, int Wd, int cin, const float* sc2,
                                                                       const float* sc1) {
    const int64_t i = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    const int C4 = cin >> 2;
    if (i >= rows * C4) return;
    const int cq = (int)(i % C4);
    const int64_t m = i / C4;
    const int HW = H * Wd, img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / Wd, x = rem - y * Wd;
    float* d = dx + (((int64_t)img * 2 * H + 2 * y) * 2 * Wd + 2 * x) * cin + 4 * cq;
    const float mul = sc2[2] * sc1[2];
    floatx4 a = *(floatx4*)d;
    const floatx4 b = *(const floatx4*)(t + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += b[e] * mul;
    *(floatx4*)d = a;
}

// the tensors of one struct the block reads: params (five per pair) or grads (the three learnable fields per pair)
int struct_check(const Fam& fam, const vtd_bottleneck_params* p, bool ds, bool stats) {
    const int err_arg = fam.err_arg, err_align = fam.err_align;
    if (!p) return err_arg;
    const float* const f[4][5] = {{p->conv1_w, p->bn1_w, p->bn1_b, p->bn1_mean, p->bn1_var}, {p->conv2_w, p->bn2_w, p->bn2_b, p->bn2_mean, p->bn2_var},
                                  {p->conv3_w, p->bn3_w, p->bn3_b, p->bn3_mean, p->bn3_var}, {p->ds_w, p->ds_bn_w, p->ds_bn_b, p->ds_bn_mean, p->ds_bn_var}};
    uintptr_t bits = 0;
    for (int i = 0; i < (ds ? 4 : 3); ++i)
        for (int j = 0; j < (stats ? 5 : 3); ++j) {
            if (!f[i][j]) return err_arg;
            bits |= (uintptr_t)f[i][j];
        }
    return (bits & 3) ? err_align : 0;
}

void padded_out(ConvParams& c, int h, int w, int ch, half_t* out) {
    c.out = out; c.out_hp = h + 2; c.out_wp = w + 2; c.out_c = ch; c.out_ring = 1;
}

unsigned ring_blocks(int n, int h, int w, int ch) { return nblk((int64_t)n * (2 * (w + 2) + 2 * h) * (ch / 8)); }

int64_t ws_bytes(const Fam& fam, int n, int hin, int win, int cin, int width, int stride, int mode) {
    Geo g;
    if (!make_geo(fam, n, hin, win, cin, width, stride, g) || mode < 0 || mode > 1) return fam.err_arg;
    return mode ? bwd_layout(g).total : fwd_layout(g).total;
}

int launch_forward(const Fam& fam, const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps, void* ws,
                   void* y, hipStream_t s) {
    const int err_arg = fam.err_arg, err_align = fam.err_align;
    Geo g;
    if (!x || !ws || !y || !make_geo(fam, n, hin, win, cin, width, stride, g) || !(eps > 0.f)) return err_arg;
    const int W = g.W, OUT = g.OUT;
    const int pc = struct_check(fam, P, g.ds, true);
    if (pc == err_arg) return pc;
    if (pc || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255)) return err_align;
    const FwdLayout L = fwd_layout(g);
    char* w = (char*)ws;
    half_t *a1 = (half_t*)(w + L.a1), *a2 = (half_t*)(w + L.a2), *id = (half_t*)(w + L.id), *w1 = (half_t*)(w + L.w1), *w2 = (half_t*)(w + L.w2),
           *w3 = (half_t*)(w + L.w3), *wd = (half_t*)(w + L.wd);
    float *b1 = (float*)(w + L.bias), *b2 = b1 + W, *b3 = b2 + W, *bd = b3 + OUT;
    auto fold = [&](const float* cw, const float* gam, const float* bet, const float* mean, const float* var, int cout, int ci, int taps, half_t* wp,
                    float* bias) {
        hipLaunchKernelGGL(rb_fold_kernel, dim3(nblk((int64_t)cout * taps * ci + cout)), dim3(RB_THREADS), 0, s, cw, gam, bet, mean, var, eps, cout, ci, taps,
                           wp, bias);
    };
    fold(P->conv1_w, P->bn1_w, P->bn1_b, P->bn1_mean, P->bn1_var, W, cin, 1, w1, b1);
    fold(P->conv2_w, P->bn2_w, P->bn2_b, P->bn2_mean, P->bn2_var, W, W, 9, w2, b2);
    fold(P->conv3_w, P->bn3_w, P->bn3_b, P->bn3_mean, P->bn3_var, OUT, W, 1, w3, b3);
    if (g.ds) fold(P->ds_w, P->ds_bn_w, P->ds_bn_b, P->ds_bn_mean, P->ds_bn_var, OUT, cin, 1, wd, bd);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, hin, win, W)), dim3(RB_THREADS), 0, s, a1, n, hin, win, W);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, W)), dim3(RB_THREADS), 0, s, a2, n, g.h, g.w, W);
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, OUT)), dim3(RB_THREADS), 0, s, (half_t*)y, n, g.h, g.w, OUT);
    VTD_HIP_CHECK(hipGetLastError());
    int rc;
    ConvParams c1 = conv_of(n, hin, win, W, (const half_t*)x, cin, hin, win, 1, 1, w1, b1);
    c1.flags = EPI_RELU;
    padded_out(c1, hin, win, W, a1);
    if ((rc = vtd_launch_conv(c1, -1, s))) return rc;
    ConvParams c2 = conv_of(n, g.h, g.w, W, a1, W, hin, win, 3, stride, w2, b2);
    c2.flags = EPI_RELU;
    padded_out(c2, g.h, g.w, W, a2);
    if ((rc = vtd_launch_conv(c2, -1, s))) return rc;
    if (g.ds) {
        ConvParams d = conv_of(n, g.h, g.w, OUT, (const half_t*)x, cin, hin, win, 1, stride, wd, bd);
        padded_out(d, g.h, g.w, OUT, id);
        if ((rc = vtd_launch_conv(d, -1, s))) return rc;
    }
    ConvParams c3 = conv_of(n, g.h, g.w, OUT, a2, W, g.h, g.w, 1, 1, w3, b3);
    c3.flags = EPI_RELU | EPI_RESIDUAL;
    c3.res = g.ds ? id : (const half_t*)x; c3.res_hp = g.h + 2; c3.res_wp = g.w + 2; c3.res_ring = 1; c3.res_shift = 0;
    padded_out(c3, g.h, g.w, OUT, (half_t*)y);
    return vtd_launch_conv(c3, -1, s);
}

int launch_backward(const Fam& fam, const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                    const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch, float* dx,
                    float* dxscale, hipStream_t s) {
    const int err_arg = fam.err_arg, err_align = fam.err_align;
    Geo g;
    if (!x || !ws || !y || !dy || !dscale || !scratch || !make_geo(fam, n, hin, win, cin, width, stride, g) || !(eps > 0.f) || (dx && !dxscale))
        return err_arg;
    const int W = g.W, OUT = g.OUT;
    const int pc = struct_check(fam, P, g.ds, true), gc = struct_check(fam, Gp, g.ds, false);
    if (pc == err_arg || gc == err_arg) return err_arg;
    if (pc || gc || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)ws & 255) || ((uintptr_t)scratch & 255) || ((uintptr_t)dy & 15) || ((uintptr_t)dscale & 7) ||
        ((uintptr_t)dx & 15) || ((uintptr_t)dxscale & 7))
        return err_align;
    const FwdLayout L = fwd_layout(g);
    const BwdLayout B = bwd_layout(g);
    char* q = (char*)scratch;
    const half_t *a1 = (const half_t*)((const char*)ws + L.a1), *a2 = (const half_t*)((const char*)ws + L.a2);
    float *g3 = (float*)(q + B.g3), *g2 = (float*)(q + B.g2), *g1 = (float*)(q + B.g1), *zero = (float*)(q + B.zero), *pmax = (float*)(q + B.pmax),
          *sc = (float*)(q + B.sc), *slab = (float*)(q + B.slab);
    half_t *g3h = (half_t*)(q + B.g3h), *g2h = (half_t*)(q + B.g2h), *g1h = (half_t*)(q + B.g1h), *g3p = (half_t*)(q + B.g3p), *g2p = (half_t*)(q + B.g2p),
           *g1p = (half_t*)(q + B.g1p), *wt = (half_t*)(q + B.wt);
    double *part = (double*)(q + B.part), *sum3 = (double*)(q + B.sum3), *sum2 = (double*)(q + B.sum2), *sum1 = (double*)(q + B.sum1);
    float *sc3 = sc, *sc2 = sc + 4, *sc1 = sc + 8;
    const int64_t M = g.m, Min = g.min;
    int rc;

    auto red_grid = [](int64_t rows, int per_wg, int64_t& per) {
        int64_t G = (rows + per_wg - 1) / per_wg;
        G = G < 1 ? 1 : G > BK_MAX_RED ? BK_MAX_RED : G;
        per = (rows + G - 1) / G;
        return (int)G;
    };
    // finish + the fp16 operands of a masked gradient `gout` [rows][C] of h x w pixels: flat, and ring-padded at pixel (dil y, dil x)
    auto finish_form = [&](const float* gout, int64_t rows, int h, int w, int C, int G, const float* in_sc, double* sum, float* out_sc, half_t* flat,
                           half_t* padded, int dil) {
        hipLaunchKernelGGL(rb_finish_kernel, dim3(1), dim3(RB_THREADS), 0, s, (const double*)part, (const float*)pmax, G, C, in_sc, sum, out_sc);
        hipLaunchKernelGGL(rb_form_kernel, dim3(nblk(rows * (C / 8))), dim3(RB_THREADS), 0, s, gout, rows, (const float*)out_sc, h, w, C, dil, flat, padded);
    };
    // a W-wide stage: v masked by the padded activation `act` of h x w pixels (in place when gout == v), reduced, formed
    auto stageW = [&](const float* v, const half_t* act, float* gout, int64_t rows, int h, int w, const float* in_sc, double* sum, float* out_sc,
                        half_t* flat, half_t* padded, int dil) {
        int64_t per;
        const int G = red_grid(rows, 256, per);
        hipLaunchKernelGGL(rb_mask_kernel, dim3(nblk(rows * (W / 4))), dim3(RB_THREADS), 0, s, v, act, rows, h, w, W, gout);
        if (W == 64)
            hipLaunchKernelGGL(rb_reduce64_kernel, dim3(G), dim3(RB_THREADS), 0, s, (const float*)gout, rows, per, part, pmax);
        else if (W == 128)
            hipLaunchKernelGGL(rb_reduce128_kernel, dim3(G), dim3(RB_THREADS), 0, s, (const float*)gout, rows, per, part, pmax);
        else
            hipLaunchKernelGGL(rb_reduce_kernel, dim3(G), dim3(RB_THREADS), 0, s, (const float*)gout, rows, per, W, part, pmax);
        finish_form(gout, rows, h, w, W, G, in_sc, sum, out_sc, flat, padded, dil);
    };
    // a: [rows][lda] gradients of a convolution of ksz x ksz at stride st over the padded input xin (xc channels, hi x wi pixels) whose output
    // has ho x wo pixels
    auto wgrad = [&](const half_t* a, int lda, int64_t rows, int ho, int wo, const half_t* xin, int xc, int hi, int wi, int ksz, int st, const float* scl,
                     const double* sum, const float* w, const float* gam, const float* mean, const float* var, float* dw, float* dgam, float* dbet) {
        WgArgs wa;
        wa.a = a; wa.lda = lda; wa.x = xin; wa.xc = xc; wa.n = n; wa.H = ho; wa.W = wo; wa.rows = rows; wa.slab = slab;
        const int nqt = wg_nqt(ksz, xc), Sl = bk_slabs(g, rows, nqt, lda);
        wa.slab_len = slab_rows(rows, Sl); wa.ksz = ksz; wa.stride = st; wa.Hin = hi; wa.Win = wi;
        if (lda == 64)   // res2's conv2 and conv1: the 64-row tile, one column tile, slab [64][ksz^2 xc]
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<5>, dim3(nqt * Sl, 1), dim3(WG_THREADS), 0, s, wa);
        else if (xc & 127)   // res2's conv3 and downsample over 64 channels: half a q-tile
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<4>, dim3(nqt * Sl, lda / 128), dim3(WG_THREADS), 0, s, wa);
        else
            hipLaunchKernelGGL(dbhead_train_wgrad_kernel<3>, dim3(nqt * Sl, lda / 128), dim3(WG_THREADS), 0, s, wa);
        hipLaunchKernelGGL(rb_param_kernel, dim3(lda), dim3(RB_THREADS), 0, s, (const float*)slab, Sl, xc, ksz * ksz, scl, sum, w, gam, mean, var, eps, dw, dgam,
                           dbet);
    };
    // conv^T of a padded gradient plane gp of hp x wp pixels and C channels into [n hp wp][rows] fp32: the folded weights of a convolution
    // with `rows` input and C output channels, rotated and transposed into the panel `wt`
    auto dgrad = [&](const half_t* gp, int hp, int wp, int C, const float* w, const float* gam, const float* var, int rows, int ksz, float* out) {
        hipLaunchKernelGGL(rb_pack_dgrad_kernel, dim3(nblk((int64_t)rows * ksz * ksz * C + C)), dim3(RB_THREADS), 0, s, w, gam, var, eps, C, rows, ksz * ksz, wt,
                           zero);
        ConvParams c = conv_of(n, hp, wp, rows, gp, C, hp, wp, ksz, 1, wt, zero);
        c.out = out; c.ldc = rows; c.flags = EPI_OUT_F32;
        return vtd_launch_conv(c, -1, s);
    };

    // the zero bias row of the transposed convolutions: up to 4 W outputs (conv1^T of the identity block)
    VTD_HIP_CHECK(hipMemsetAsync(zero, 0, OUT * 4, s));
    {   // g3 = dy (y > 0), 4 W wide
        int64_t per;
        const int G = red_grid(M, 32, per);
        if (OUT == 2048)
            hipLaunchKernelGGL(bk_mask_reduce_kernel<2>, dim3(G), dim3(RB_THREADS), 0, s, dy, (const half_t*)y, M, per, g.h, g.w, g3, part, pmax);
        else if (OUT == 1024)
            hipLaunchKernelGGL(bk_mask_reduce_kernel<1>, dim3(G), dim3(RB_THREADS), 0, s, dy, (const half_t*)y, M, per, g.h, g.w, g3, part, pmax);
        else if (OUT == 512)
            hipLaunchKernelGGL(bk_mask_reduce512_kernel, dim3(G), dim3(RB_THREADS), 0, s, dy, (const half_t*)y, M, per, g.h, g.w, g3, part, pmax);
        else
            hipLaunchKernelGGL(bk_mask_reduce256_kernel, dim3(G), dim3(RB_THREADS), 0, s, dy, (const half_t*)y, M, per, g.h, g.w, g3, part, pmax);
        hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, OUT)), dim3(RB_THREADS), 0, s, g3p, n, g.h, g.w, OUT);
        finish_form(g3, M, g.h, g.w, OUT, G, dscale, sum3, sc3, g3h, g3p, 1);
    }
    VTD_HIP_CHECK(hipGetLastError());
    wgrad(g3h, OUT, M, g.h, g.w, a2, W, g.h, g.w, 1, 1, sc3, sum3, P->conv3_w, P->bn3_w, P->bn3_mean, P->bn3_var, Gp->conv3_w, Gp->bn3_w, Gp->bn3_b);
    if (g.ds)
        wgrad(g3h, OUT, M, g.h, g.w, (const half_t*)x, cin, hin, win, 1, stride, sc3, sum3, P->ds_w, P->ds_bn_w, P->ds_bn_mean, P->ds_bn_var, Gp->ds_w,
              Gp->ds_bn_w, Gp->ds_bn_b);
    VTD_HIP_CHECK(hipGetLastError());
    // da2 = conv3^T(g3) into the g2 buffer, masked in place by a2 > 0.  Its padded operand is of the input's extent: the interior for the
    // stride-1 block, the even positions of a zeroed plane for the stride-2 block
    if ((rc = dgrad(g3p, g.h, g.w, OUT, P->conv3_w, P->bn3_w, P->bn3_var, W, 1, g2))) return rc;
    if (stride == 2)
        VTD_HIP_CHECK(hipMemsetAsync(g2p, 0, (size_t)g.pin * W * 2, s));
    else
        hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, g.h, g.w, W)), dim3(RB_THREADS), 0, s, g2p, n, g.h, g.w, W);
    stageW(g2, a2, g2, M, g.h, g.w, sc3, sum2, sc2, g2h, g2p, stride);
    wgrad(g2h, W, M, g.h, g.w, a1, W, hin, win, 3, stride, sc2, sum2, P->conv2_w, P->bn2_w, P->bn2_mean, P->bn2_var, Gp->conv2_w, Gp->bn2_w, Gp->bn2_b);
    VTD_HIP_CHECK(hipGetLastError());
    // da1 = conv2^T(g2) at the input's extent into the g1 buffer, masked in place by a1 > 0
    if ((rc = dgrad(g2p, hin, win, W, P->conv2_w, P->bn2_w, P->bn2_var, W, 3, g1))) return rc;
    hipLaunchKernelGGL(rb_zero_ring_kernel, dim3(ring_blocks(n, hin, win, W)), dim3(RB_THREADS), 0, s, g1p, n, hin, win, W);
    stageW(g1, a1, g1, Min, hin, win, sc2, sum1, sc1, g1h, g1p, 1);
    wgrad(g1h, W, Min, hin, win, (const half_t*)x, cin, hin, win, 1, 1, sc1, sum1, P->conv1_w, P->bn1_w, P->bn1_mean, P->bn1_var, Gp->conv1_w, Gp->bn1_w,
          Gp->bn1_b);
    VTD_HIP_CHECK(hipGetLastError());
    if (dx) {
        if ((rc = dgrad(g1p, hin, win, W, P->conv1_w, P->bn1_w, P->bn1_var, cin, 1, dx))) return rc;
        if (!g.ds) {
            hipLaunchKernelGGL(bk_add_identity_kernel, dim3(nblk(M * (OUT / 4))), dim3(RB_THREADS), 0, s, dx, (const float*)g3, M * (OUT / 4),
                               (const float*)sc3, (const float*)sc2, (const float*)sc1);
        } else {
            // ds^T(g3) at g3's scale into the g3 buffer (its fp32 values are in the operands by now), then onto the even positions; res2.0's
            // downsample has stride 1, so its term is dense: every pixel, the same two multipliers (rb_add_identity_kernel's sum)
            if ((rc = dgrad(g3p, g.h, g.w, OUT, P->ds_w, P->ds_bn_w, P->ds_bn_var, cin, 1, g3))) return rc;
            if (stride == 2)
                hipLaunchKernelGGL(bk_add_downsample_kernel, dim3(nblk(M * (cin / 4))), dim3(RB_THREADS), 0, s, dx, (const float*)g3, M, g.h, g.w, cin,
                                   (const float*)sc2, (const float*)sc1);
            else
                hipLaunchKernelGGL(rb_add_identity_kernel, dim3(nblk(M * (cin / 4))), dim3(RB_THREADS), 0, s, dx, (const float*)g3, M * (cin / 4),
                                   (const float*)sc2, (const float*)sc1);
        }
        hipLaunchKernelGGL(rb_copy_scale_kernel, dim3(1), dim3(64), 0, s, (const float*)sc1, dxscale);
    }
    return -(int)hipGetLastError();
}

}  // namespace

int64_t vtd_bottleneck_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(BK_RES5, n, hin, win, cin, width, stride, mode);
}

int vtd_launch_bottleneck_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps, void* ws,
                                  void* y, hipStream_t s) {
    return launch_forward(BK_RES5, x, n, hin, win, cin, width, stride, P, eps, ws, y, s);
}

int vtd_launch_bottleneck_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                   const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                   float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(BK_RES5, x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
}

// res4 (torchvision's layer3), W = 256: (512 -> 256 -> 1024, stride 2, downsample) and (1024 -> 256 -> 1024, stride 1, identity)
int64_t vtd_bottleneck256_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(BK_RES4, n, hin, win, cin, width, stride, mode);
}

int vtd_launch_bottleneck256_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                     void* ws, void* y, hipStream_t s) {
    return launch_forward(BK_RES4, x, n, hin, win, cin, width, stride, P, eps, ws, y, s);
}

int vtd_launch_bottleneck256_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                      const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                      float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(BK_RES4, x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
}

// res3 (torchvision's layer2), W = 128: (256 -> 128 -> 512, stride 2, downsample) and (512 -> 128 -> 512, stride 1, identity)
int64_t vtd_bottleneck128_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(BK_RES3, n, hin, win, cin, width, stride, mode);
}

int vtd_launch_bottleneck128_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                     void* ws, void* y, hipStream_t s) {
    return launch_forward(BK_RES3, x, n, hin, win, cin, width, stride, P, eps, ws, y, s);
}

int vtd_launch_bottleneck128_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                      const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                      float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(BK_RES3, x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
}

// res2 (torchvision's layer1), W = 64: (64 -> 64 -> 256, stride 1, downsample at stride 1) and (256 -> 64 -> 256, stride 1, identity)
int64_t vtd_bottleneck64_ws_bytes(int n, int hin, int win, int cin, int width, int stride, int mode) {
    return ws_bytes(BK_RES2, n, hin, win, cin, width, stride, mode);
}

int vtd_launch_bottleneck64_forward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                    void* ws, void* y, hipStream_t s) {
    return launch_forward(BK_RES2, x, n, hin, win, cin, width, stride, P, eps, ws, y, s);
}

int vtd_launch_bottleneck64_backward(const void* x, int n, int hin, int win, int cin, int width, int stride, const vtd_bottleneck_params* P, float eps,
                                     const void* ws, const void* y, const float* dy, const float* dscale, const vtd_bottleneck_params* Gp, void* scratch,
                                     float* dx, float* dxscale, hipStream_t s) {
    return launch_backward(BK_RES2, x, n, hin, win, cin, width, stride, P, eps, ws, y, dy, dscale, Gp, scratch, dx, dxscale, s);
}
