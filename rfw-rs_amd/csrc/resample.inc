// resample.inc — the render scale's one stage (DESIGN.md "Render scale"): the finalised frame of the RENDER size -> the frame of the WINDOW
// size, behind whichever of launch_assemble / launch_ao_filter / launch_atrous wrote it and before the 2D layer; included by kernels.hip
// inside namespace rfwhip.  It runs only where the two sizes differ.  The filter's definition (include/rfw_hip.h, option "scale_filter") is
// integers and single IEEE operations, so that a restatement elsewhere can be bit-exact.
//
// Per axis — R the render extent, N the window extent, x the window index — an ordered tap list (source index, weight):
//   nearest   (filter 0)         [(((2x + 1) R) / (2N), 1)]
//   bilinear  (filter 1, R <= N) num = (2x + 1) R - N;  num < 0: [(0, 1)];  else i0 = num / 2N, f = (float)(num % 2N) / (float)(2N);
//                                f == 0 or i0 == R - 1: [(i0, 1)];  else [(i0, 1 - f), (i0 + 1, f)]
//   area      (filter 1, R > N)  j = (x R) / N ... ((x + 1) R - 1) / N, weight (float)o_j / (float)R with the overlap
//                                o_j = min((x + 1) R, (j + 1) N) - max(x R, j N): at most kRsMaxTaps taps at scale <= 4
// A list's value per channel is s = v_0 w_0, then s = s + v_k w_k in list order; a list of ONE tap (its weight is 1) copies.  A window pixel
// is the vertical list over the horizontal results of its source rows.  No tap of weight zero exists: a NaN stays inside its footprint.
//
// k_resample: one thread per window pixel of a row, a wavefront = 64 consecutive pixels (1 KiB stores); a workgroup walks rows
// blockIdx.y, + gridDim.y, ...: the horizontal list is made once per thread, the vertical one is the same for the whole workgroup (scalar
// registers).  The tap loops are unrolled over kRsMaxTaps with the weights in registers: no LDS, no scratch.

constexpr uint32_t kRsMaxTaps = 5;

struct RsAxis {
    uint32_t first, count; // source indices first ... first + count - 1
    uint32_t kind;         // 0: one tap, a copy; 1: bilinear pair (1 - f, f); 2: area
    float f;
};

// T: unsigned 32 bits where (2N + 1) R fits, else 64 (launch_resample)
template <typename T> RFW_DI RsAxis rs_axis(const uint32_t R, const uint32_t N, const uint32_t x, const uint32_t filter)
{
    RsAxis a;
    a.kind = 0u; a.count = 1u; a.f = 0.0f;
    if (filter == 0u) {
        a.first = (uint32_t)((((T)2 * x + 1u) * R) / ((T)2 * N));
    } else if (R <= N) {
        const T odd = ((T)2 * x + 1u) * R;
        if (odd < (T)N) {
            a.first = 0u;
        } else {
            const T num = odd - N, den = (T)2 * N;
            a.first = (uint32_t)(num / den);
            const float f = (float)(num % den) / (float)den;
            if (f != 0.0f && a.first != R - 1u) { a.kind = 1u; a.count = 2u; a.f = f; }
        }
    } else {
        a.first = (uint32_t)(((T)x * R) / N);
        a.count = (uint32_t)((((T)x + 1u) * R - 1u) / N) - a.first + 1u;
        a.kind = 2u;
    }
    return a;
}
// weight of tap k (< a.count) of a list of more than one tap
template <typename T> RFW_DI float rs_weight(const RsAxis& a, const uint32_t R, const uint32_t N, const uint32_t x, const uint32_t k)
{
    if (a.kind == 1u) return k == 0u ? 1.0f - a.f : a.f;
    const T j = (T)a.first + k;
    const T lo = (T)x * R, hi = ((T)x + 1u) * R, jl = j * N, jh = (j + 1u) * N;
    const T o = (hi < jh ? hi : jh) - (lo > jl ? lo : jl);
    return (float)o / (float)R;
}

struct RsFrame {
    uint32_t rw, rh; // source: the render size
    uint32_t w, h;   // destination: the window size
    uint32_t filter;
};

template <typename T> RFW_DI void rs_body(const RsFrame f, const float4* __restrict__ src, float4* __restrict__ dst)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= f.w) return;
    src += (size_t)blockIdx.z * f.rw * f.rh;
    dst += (size_t)blockIdx.z * f.w * f.h;
    const RsAxis ax = rs_axis<T>(f.rw, f.w, x, f.filter);
    float wx[kRsMaxTaps];
#pragma unroll
    for (uint32_t k = 0; k < kRsMaxTaps; k++) wx[k] = (ax.count > 1u && k < ax.count) ? rs_weight<T>(ax, f.rw, f.w, x, k) : 1.0f;
    for (uint32_t y = blockIdx.y; y < f.h; y += gridDim.y) {
        const RsAxis ay = rs_axis<T>(f.rh, f.h, y, f.filter);
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (uint32_t ky = 0; ky < ay.count; ky++) {
            const float4* row = src + (size_t)(ay.first + ky) * f.rw + ax.first;
            float4 r = row[0];
            if (ax.count > 1u) {
                r.x = r.x * wx[0]; r.y = r.y * wx[0]; r.z = r.z * wx[0]; r.w = r.w * wx[0];
#pragma unroll
                for (uint32_t k = 1; k < kRsMaxTaps; k++)
                    if (k < ax.count) {
                        const float4 v = row[k];
                        r.x = r.x + v.x * wx[k]; r.y = r.y + v.y * wx[k]; r.z = r.z + v.z * wx[k]; r.w = r.w + v.w * wx[k];
                    }
            }
            if (ay.count == 1u) s = r;
            else {
                const float wy = rs_weight<T>(ay, f.rh, f.h, y, ky);
                if (ky == 0u) { s.x = r.x * wy; s.y = r.y * wy; s.z = r.z * wy; s.w = r.w * wy; }
                else { s.x = s.x + r.x * wy; s.y = s.y + r.y * wy; s.z = s.z + r.z * wy; s.w = s.w + r.w * wy; }
            }
        }
        dst[(size_t)y * f.w + x] = s;
    }
}
__global__ __launch_bounds__(256) void k_resample(const RsFrame f, const float4* __restrict__ src, float4* __restrict__ dst) { rs_body<uint32_t>(f, src, dst); }
__global__ __launch_bounds__(256) void k_resample_wide(const RsFrame f, const float4* __restrict__ src, float4* __restrict__ dst) { rs_body<uint64_t>(f, src, dst); }

void launch_resample(hipStream_t s, const float4* src, uint32_t rw, uint32_t rh, float4* dst, uint32_t w, uint32_t h, uint32_t filter, uint32_t frames)
{
    if (!w || !h || !rw || !rh || !frames) return;
    const RsFrame f{rw, rh, w, h, filter};
    const uint32_t bx = (w + 255u) / 256u;
    // a memory stream: some 2048 workgroups, each walking its share of the rows (and making its horizontal lists once)
    const dim3 grid(bx, std::min(h, std::max(1u, 2048u / bx)), frames);
    const uint64_t top = (2ull * std::max(w, h) + 1ull) * std::max(rw, rh);
    if (top < (1ull << 32)) hipLaunchKernelGGL(k_resample, grid, dim3(256), 0, s, f, src, dst);
    else hipLaunchKernelGGL(k_resample_wide, grid, dim3(256), 0, s, f, src, dst);
}
