// AdamW parameter update (trainer.py:107-112: torch.optim.AdamW(self.parameters(), lr, weight_decay)), one multi-tensor pass.
//
// Per element, all fp32, every operation rounded once (this file is built with -ffp-contract=off: no fused multiply-add), in torch's
// order (decoupled decay, lerp form of the first moment, mul + addcmul of the second, sqrt / bias correction + eps, addcdiv):
//     p1  = p * decay                              decay = 1 - lr * weight_decay
//     m'  = m + one_minus_beta1 * (g - m)
//     v'  = v * beta2 + (one_minus_beta2 * g) * g
//     den = sqrt(v') / bc2_sqrt + eps              bc2_sqrt = sqrt(1 - beta2^step)
//     p'  = p1 - step_size * (m' / den)            step_size = lr / (1 - beta1^step)
// IEEE division and square root, subnormals kept (the compiler's defaults for fp32 on gfx950).
//
// HBM-bound: 16 B read and 12 B written per element (p, g, m, v in; p, m, v out), nothing else.  The tensor table travels in the kernel
// arguments, 64 tensors (3 KB) a launch, with the prefix of their chunk counts behind it: nothing is staged in device memory, nothing
// outlives the call, the host never waits.  A workgroup takes chunks of VTD_ADAMW_CHUNK elements: chunk w of the slice belongs to the
// tensor t with prefix[t] <= w < prefix[t + 1], found by a binary search on wave-uniform values (scalar loads of the argument segment,
// scalar compares).  Element-wise, no atomics, the grid a function of the n values only: bitwise repeatable.
#include "vtd_common.h"
#include "../../include/vtd.h"

namespace {

constexpr int AW_THREADS = 256;
constexpr int AW_MAX_BLOCKS = 2048;                          // 256 CUs x 8; the rest is strided
constexpr int AW_VECS = VTD_ADAMW_CHUNK / (AW_THREADS * 4);   // 16-byte accesses per lane, array and chunk
static_assert(VTD_ADAMW_CHUNK % 1024 == 0 && AW_VECS >= 1, "a chunk is whole rows of 256 lanes x 4 floats");
static_assert(sizeof(vtd_adamw_tensor) == 48, "64 entries and the prefix must fit the 4 KB argument segment");

struct AdamwSlice {
    vtd_adamw_tensor t[VTD_ADAMW_SLICE];
    int64_t prefix[VTD_ADAMW_SLICE + 1];   // prefix[i] = chunks of tensors 0 .. i-1; entries past `count` repeat the total
    vtd_adamw_hyper h;
    int count;
};
static_assert(sizeof(AdamwSlice) <= 4096, "kernel arguments");

struct Pmv {
    float p, m, v;
};

__device__ __forceinline__ Pmv adamw_element(float p, float g, float m, float v, const vtd_adamw_hyper& h, float step_size, float bc2_sqrt) {
    const float p1 = p * h.decay;
    const float m1 = m + h.one_minus_beta1 * (g - m);
    const float v1 = v * h.beta2 + (h.one_minus_beta2 * g) * g;
    const float den = sqrtf(v1) / bc2_sqrt + h.eps;
    return Pmv{p1 - step_size * (m1 / den), m1, v1};
}

__global__ __launch_bounds__(AW_THREADS) void adamw_kernel(const AdamwSlice s) {
    const int64_t total = s.prefix[s.count];
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        int lo = 0, hi = s.count;   // prefix[lo] <= w < prefix[hi]; tensors of no chunk (n == 0) are never landed on
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s.prefix[mid] <= w) lo = mid; else hi = mid;
        }
        const vtd_adamw_tensor& t = s.t[lo];
        const int64_t base = (w - s.prefix[lo]) * VTD_ADAMW_CHUNK;
        const int64_t left = t.n - base;   // >= 1
        float* const p = t.p + base;
        const float* const g = t.g + base;
        float* const m = t.m + base;
        float* const v = t.v + base;
        const float step_size = t.step_size, bc2_sqrt = t.bc2_sqrt;
        const bool aligned = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0);   // a chunk is a multiple of 16 B
        if (aligned && left >= VTD_ADAMW_CHUNK) {
            // a whole chunk: every load of the lane in flight before the first use
            floatx4 a[AW_VECS], b[AW_VECS], c[AW_VECS], d[AW_VECS];
#pragma unroll
            for (int k = 0; k < AW_VECS; ++k) {
                const int i = (k * AW_THREADS + threadIdx.x) * 4;
                a[k] = *(const floatx4*)(p + i);
                b[k] = *(const floatx4*)(g + i);
                c[k] = *(const floatx4*)(m + i);
                d[k] = *(const floatx4*)(v + i);
            }
#pragma unroll
            for (int k = 0; k < AW_VECS; ++k) {
                const int i = (k * AW_THREADS + threadIdx.x) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const Pmv r = adamw_element(a[k][e], b[k][e], c[k][e], d[k][e], s.h, step_size, bc2_sqrt);
                    a[k][e] = r.p;
                    c[k][e] = r.m;
                    d[k][e] = r.v;
                }
                *(floatx4*)(p + i) = a[k];
                *(floatx4*)(m + i) = c[k];
                *(floatx4*)(v + i) = d[k];
            }
        } else if (aligned) {
            // the tensor's last chunk: whole float4 groups, then the n % 4 elements one lane each
            const int len = (int)left, len4 = len >> 2;
            for (int q = threadIdx.x; q < len4; q += AW_THREADS) {
                floatx4 a = *(const floatx4*)(p + 4 * q), c = *(const floatx4*)(m + 4 * q), d = *(const floatx4*)(v + 4 * q);
                const floatx4 b = *(const floatx4*)(g + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const Pmv r = adamw_element(a[e], b[e], c[e], d[e], s.h, step_size, bc2_sqrt);
                    a[e] = r.p;
                    c[e] = r.m;
                    d[e] = r.v;
                }
                *(floatx4*)(p + 4 * q) = a;
                *(floatx4*)(m + 4 * q) = c;
                *(floatx4*)(v + 4 * q) = d;
            }
            const int i = (len4 << 2) + threadIdx.x;
            if (i < len) {
                const Pmv r = adamw_element(p[i], g[i], m[i], v[i], s.h, step_size, bc2_sqrt);
                p[i] = r.p;
                m[i] = r.m;
                v[i] = r.v;
            }
        } else {
            // a tensor that is 4- but not 16-byte aligned (a view that starts mid-row): dword accesses, still coalesced
            const int len = left < VTD_ADAMW_CHUNK ? (int)left : VTD_ADAMW_CHUNK;
            for (int i = threadIdx.x; i < len; i += AW_THREADS) {
                const Pmv r = adamw_element(p[i], g[i], m[i], v[i], s.h, step_size, bc2_sqrt);
                p[i] = r.p;
                m[i] = r.m;
                v[i] = r.v;
            }
        }
    }
}

bool finite_f(float x) { return x - x == 0.0f; }   // false for NaN and +-Inf

}  // namespace

int vtd_launch_adamw(const vtd_adamw_tensor* tensors, int count, const vtd_adamw_hyper* hyper, hipStream_t stream) {
    if (count < 0) return -3601;
    if (count == 0) return 0;
    if (!tensors || !hyper) return -3601;
    if (!finite_f(hyper->decay) || !finite_f(hyper->one_minus_beta1) || !finite_f(hyper->beta2) || !finite_f(hyper->one_minus_beta2) ||
        !finite_f(hyper->eps))
        return -3601;
    // the whole table is checked before the first launch
    for (int i = 0; i < count; ++i) {
        const vtd_adamw_tensor& t = tensors[i];
        if (t.n < 0 || t.n >= ((int64_t)1 << 40)) return -3601;
        if (!finite_f(t.bc2_sqrt) || !(t.bc2_sqrt > 0.0f) || !finite_f(t.step_size)) return -3601;
        if (t.n == 0) continue;   // skipped: its pointers are never looked at
        if (!t.p || !t.g || !t.m || !t.v) return -3601;
        if (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 3) return -3601;
    }
    for (int first = 0; first < count; first += VTD_ADAMW_SLICE) {
        AdamwSlice s;
        s.count = count - first < VTD_ADAMW_SLICE ? count - first : VTD_ADAMW_SLICE;
        s.h = *hyper;
        s.prefix[0] = 0;
        for (int i = 0; i < VTD_ADAMW_SLICE; ++i) {
            if (i < s.count) {
                s.t[i] = tensors[first + i];
                s.prefix[i + 1] = s.prefix[i] + (s.t[i].n + VTD_ADAMW_CHUNK - 1) / VTD_ADAMW_CHUNK;
            } else {
                s.t[i] = vtd_adamw_tensor{nullptr, nullptr, nullptr, nullptr, 0, 0.0f, 1.0f};
                s.prefix[i + 1] = s.prefix[i];
            }
        }
        const int64_t total = s.prefix[s.count];
        if (total == 0) continue;
        // grid: a function of the n values only; one workgroup per chunk up to 256 CUs x 8, which then stride the rest
        const unsigned blocks = (unsigned)(total < AW_MAX_BLOCKS ? total : AW_MAX_BLOCKS);
        hipLaunchKernelGGL(adamw_kernel, dim3(blocks), dim3(AW_THREADS), 0, stream, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return -(int)e;
    }
    return 0;
}
