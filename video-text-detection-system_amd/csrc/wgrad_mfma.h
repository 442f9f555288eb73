// Weight gradients of the training kernels (dbhead_train.hip, fpn_train.hip): C[p][q] = sum_m A[m][p] B[m][q] over one slab of rows, on
// v_mfma_f32_16x16x32_f16.  A is a dense fp16 matrix [rows][lda] of scaled output gradients, B is gathered from an NHWC fp16 tensor.
// MODE 0 (conv 3x3): A = 128 columns from column 128 * blockIdx.y (the DB head's dy1 [M1][128]: gridDim.y = 1; the FPN's dP2 [M][256]:
//   gridDim.y = 2), B = im2col of the ring-padded 256-channel input, q-tile qt = 128 channels of tap qt / 2: 18 q-tiles.
// MODE 1 (ConvT1): A = a1 columns of branch qt / 2 (P_T = 64), B = dz of that branch at pixel (2y+ky, 2x+kx), q = tap * 64 + co, two taps
//   per q-tile: 4 q-tiles.
// MODE 2 (conv 1x1, the FPN laterals): A as MODE 0, B = the centre pixel of a ring-padded tensor of xc channels (a multiple of 64),
//   q-tile qt = channels 128 qt .. 128 qt + 127; columns at or past xc load zeros and are not stored (ResNet-18's C2 has 64 channels).
// MODE 3 (a ResNet block's convolutions): A as MODE 0 with gridDim.y = lda / 128 column tiles (four for layer4's 512-wide gradient, two for
//   layer3's 256-wide one: the width is the launch's grid and `lda`, not a template argument), B = the ksz x ksz
//   window (ksz = 3: pad 1, ksz = 1: pad 0) at stride `stride` of a ring-padded input of xc channels (a multiple of 128) and Hin x Win
//   pixels; q = tap * xc + ci, q-tile qt = 128 channels of tap 128 qt / xc: ksz^2 xc / 128 q-tiles.  slab [128 gridDim.y][ksz^2 xc].
// MODE 4 (a ResNet block's convolutions over a 64-channel input, layer2.0's conv1 and downsample): as MODE 3 with xc a multiple of 64 that is
//   no multiple of 128.  Each 64-column group of a q-tile decodes its own tap, as MODE 1's `grp` does: group 2 qt + grp holds channels
//   (128 qt + 64 grp) % xc of tap (128 qt + 64 grp) / xc, so with xc = 64 a q-tile holds two taps.  ceil(ksz^2 xc / 128) q-tiles; columns at
//   or past ksz^2 xc (the second half of the last q-tile: K = 576 is 4.5 q-tiles, K = 64 half of one) load zeros and are not stored, as
//   MODE 2's.  slab [128 gridDim.y][ksz^2 xc].
// MODE 5 (a 64-wide ResNet block's 3x3 convolutions, layer1's): A = the 64 columns of a 64-wide gradient (lda = 64, gridDim.y = 1) on
//   MODE 1's 64-row tile (P_T = 64), B decoded as MODE 4's (xc = 64: a tap per 64-column group, K = 576 = 4.5 q-tiles, columns at or
//   past K load zeros and are not stored).  slab [64][ksz^2 xc]: the slab stride is 64 rows, not 128 gridDim.y.
// Workgroup = 4 waves, one (q-tile, slab); each wave a (P_T / 2) x 64 block.  Per K chunk of 32 rows every thread loads rows 8o .. 8o+7
// of one column pair of A and B with 4-byte loads (the next chunk's loads are in flight during this chunk's MFMAs), transposes them into
// LDS as [row octet][column][8] so that a fragment (8 consecutive rows of one column) is one 16-byte read, double-buffered: one barrier
// per chunk.  Rows past the slab load zeros.  slab[s][P][Q] fp32: MODE 0 [128 gridDim.y][2304], MODE 1 [2][64][256], MODE 2
// [128 gridDim.y][xc].
#ifndef VTD_WGRAD_MFMA_H
#define VTD_WGRAD_MFMA_H
#include "vtd_common.h"

namespace {   // per translation unit, as every kernel of this library

constexpr int WG_THREADS = 256;
constexpr int WG_KC = 32;   // rows per K chunk (one v_mfma_f32_16x16x32_f16 K-step)

struct WgArgs {
    const half_t* a;    // [rows][lda]
    int lda;
    const half_t* x;    // MODE 0: padded 256-channel input; MODE 1: dz [M2][128]; MODE 2: padded input of xc channels
    int xc;             // MODE 2: channels of x
    int n, H, W;
    int64_t rows, slab_len;
    float* slab;
    int ksz, stride, Hin, Win;   // MODES 3, 4 and 5 only
};

template <int MODE>
__device__ __forceinline__ const half_t* wg_brow(const WgArgs& A, int img, int y, int xx, int qt, int grp) {
    if constexpr (MODE == 0) {
        const int tap = qt >> 1, ky = tap / 3, kx = tap % 3;
        return A.x + (((int64_t)img * (A.H + 2) + y + ky) * (A.W + 2) + xx + kx) * 256 + (qt & 1) * 128 + grp * 64;
    } else if constexpr (MODE == 1) {
        const int b = qt >> 1, tap = (qt & 1) * 2 + grp, ky = tap >> 1, kx = tap & 1;
        return A.x + (((int64_t)img * 2 * A.H + 2 * y + ky) * 2 * A.W + 2 * xx + kx) * 128 + b * 64;
    } else if constexpr (MODE == 2) {
        return A.x + (((int64_t)img * (A.H + 2) + y + 1) * (A.W + 2) + xx + 1) * A.xc + qt * 128 + grp * 64;
    } else if constexpr (MODE == 3) {
        const int q0 = qt * 128, tap = q0 / A.xc, c0 = q0 - tap * A.xc, ky = tap / A.ksz, kx = tap - ky * A.ksz, o = 1 - (A.ksz >> 1);
        return A.x + (((int64_t)img * (A.Hin + 2) + y * A.stride + ky + o) * (A.Win + 2) + xx * A.stride + kx + o) * A.xc + c0 + grp * 64;
    } else {   // MODES 4 and 5
        const int q0 = qt * 128 + grp * 64, tap = q0 / A.xc, c0 = q0 - tap * A.xc, ky = tap / A.ksz, kx = tap - ky * A.ksz, o = 1 - (A.ksz >> 1);
        return A.x + (((int64_t)img * (A.Hin + 2) + y * A.stride + ky + o) * (A.Win + 2) + xx * A.stride + kx + o) * A.xc + c0;
    }
}

template <int MODE>
__global__ __launch_bounds__(WG_THREADS) void dbhead_train_wgrad_kernel(const WgArgs A) {
    constexpr int PT = (MODE == 1 || MODE == 5) ? 64 : 128, QT = 128, FP = PT / 32, FQ = 4;
    const int NQT = MODE == 0 ? 18 : MODE == 1 ? 4 : MODE == 2 ? (A.xc + 127) / 128 : MODE == 3 ? A.ksz * A.ksz * A.xc / 128
                                                                                       : (A.ksz * A.ksz * A.xc + 127) / 128;
    const int qt = blockIdx.x % NQT, sl = blockIdx.x / NQT, pt = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wp = w >> 1, wq = w & 1;
    const int a_col0 = MODE == 1 ? (qt >> 1) * 128 : MODE == 5 ? 0 : pt * 128;   // MODE 1: the hi half of the branch's a1 pair
    __shared__ __attribute__((aligned(16))) half_t lds[2][4 * (PT + QT) * 8];

    const int64_t r0 = (int64_t)sl * A.slab_len;
    const int64_t r1 = r0 + A.slab_len < A.rows ? r0 + A.slab_len : A.rows;
    const int nchunks = r1 > r0 ? (int)((r1 - r0 + WG_KC - 1) / WG_KC) : 0;

    // this thread's load slots: A column pair ap (octet ao), B column pair bp (octet bo)
    const int ap = t % (PT / 2), ao = t / (PT / 2);          // ao < 4 active (MODE 1: 8 octets per pass, only 4 needed)
    const int bp = t % (QT / 2), bo = t / (QT / 2);          // bo in 0..3
    const bool a_act = ao < 4;
    const int bgrp = (2 * bp) / 64, bcol = (2 * bp) % 64;
    const bool b_act = MODE == 2 ? qt * 128 + bgrp * 64 < A.xc : (MODE == 4 || MODE == 5) ? qt * 128 + bgrp * 64 < A.ksz * A.ksz * A.xc : true;
    const int HW = A.H * A.W;

    uint32_t ra[8], rb[8];
    auto gload = [&](int ch) {
        const int64_t base = r0 + (int64_t)ch * WG_KC;
        // A: rows base + 8 ao + j, columns a_col0 + 2 ap, +1
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t m = base + 8 * ao + j;
            ra[j] = (a_act && m < r1) ? *(const uint32_t*)(A.a + m * A.lda + a_col0 + 2 * ap) : 0u;
        }
        // B: rows base + 8 bo + j (consecutive: decode the first, then step x)
        int64_t m = base + 8 * bo;
        int img = (int)(m / HW), rem = (int)(m - (int64_t)img * HW), y = rem / A.W, xx = rem - y * A.W;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            rb[j] = (b_act && m < r1) ? *(const uint32_t*)(wg_brow<MODE>(A, img, y, xx, qt, bgrp) + bcol) : 0u;
            ++m;
            if (++xx == A.W) { xx = 0; if (++y == A.H) { y = 0; ++img; } }
        }
    };
    auto lstore = [&](int buf) {
        half_t* la = lds[buf];
        half_t* lb = lds[buf] + 4 * PT * 8;
        if (a_act) {
            half8 lo, hi;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lo[j] = __builtin_bit_cast(half2v, ra[j])[0];
                hi[j] = __builtin_bit_cast(half2v, ra[j])[1];
            }
            *(half8*)(la + (ao * PT + 2 * ap) * 8) = lo;
            *(half8*)(la + (ao * PT + 2 * ap + 1) * 8) = hi;
        }
        half8 lo, hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            lo[j] = __builtin_bit_cast(half2v, rb[j])[0];
            hi[j] = __builtin_bit_cast(half2v, rb[j])[1];
        }
        *(half8*)(lb + (bo * QT + 2 * bp) * 8) = lo;
        *(half8*)(lb + (bo * QT + 2 * bp + 1) * 8) = hi;
    };

    floatx4 acc[FP][FQ];
#pragma unroll
    for (int i = 0; i < FP; ++i)
#pragma unroll
        for (int j = 0; j < FQ; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    if (nchunks > 0) gload(0);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        lstore(buf);
        __syncthreads();
        if (ch + 1 < nchunks) gload(ch + 1);
        const half_t* la = lds[buf];
        const half_t* lb = lds[buf] + 4 * PT * 8;
        const int oct = lane >> 4, col = lane & 15;
        half8 fa[FP], fb[FQ];
#pragma unroll
        for (int i = 0; i < FP; ++i) fa[i] = *(const half8*)(la + (oct * PT + wp * (PT / 2) + i * 16 + col) * 8);
#pragma unroll
        for (int j = 0; j < FQ; ++j) fb[j] = *(const half8*)(lb + (oct * QT + wq * 64 + j * 16 + col) * 8);
#pragma unroll
        for (int i = 0; i < FP; ++i)
#pragma unroll
            for (int j = 0; j < FQ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }

    // C row p = wp * PT/2 + i*16 + 4*(lane>>4) + e, column q = wq*64 + j*16 + (lane&15)
    const int ldq = MODE == 0 ? 2304 : MODE == 1 ? 256 : MODE == 2 ? A.xc : A.ksz * A.ksz * A.xc;
    const int64_t slab_elems = MODE == 1 ? 2 * 64 * 256 : MODE == 5 ? (int64_t)64 * ldq : (int64_t)gridDim.y * 128 * ldq;
    float* out = A.slab + (int64_t)sl * slab_elems;
    const int p_base = MODE == 1 ? (qt >> 1) * 64 : MODE == 5 ? 0 : pt * 128;
    const int q_base = MODE == 1 ? (qt & 1) * 128 : qt * 128;
#pragma unroll
    for (int i = 0; i < FP; ++i)
#pragma unroll
        for (int j = 0; j < FQ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = p_base + wp * (PT / 2) + i * 16 + 4 * (lane >> 4) + e;
                const int q = q_base + wq * 64 + j * 16 + (lane & 15);
                if ((MODE != 2 && MODE != 4 && MODE != 5) || q < ldq) out[(int64_t)p * ldq + q] = acc[i][j][e];
            }
}

}  // namespace

#endif  // VTD_WGRAD_MFMA_H
