// display.inc — the display transform (DESIGN.md "Display transform", include/rfw_hip.h option "tonemap"): exposure, automatic exposure and a
// tone-map curve over the finalised frame of a path-traced image, in place at the RENDER size, behind whichever of launch_assemble /
// launch_atrous wrote it and before the render scale and the 2D layer; included by kernels.hip inside namespace rfwhip.  With the option off
// nothing here is launched.  Every step is integers and single IEEE operations, so that a restatement elsewhere can be bit-exact.
//
// The frame is gamma-2 (blit.comp: sqrt(acc / samples)): lin = c * c per channel, Y = 0.2126 r + 0.7152 g + 0.0722 b (left to right).
//   k_display_hist     256 bins of 1/8 octave over [2^-16, 2^16): a pixel counts iff Y >= 2^-16, bin = min(255, (bits(Y) >> 20) - 888) — the
//                      float's exponent and top three mantissa bits ARE the piecewise-linear log2, no logarithm.  Grid-stride over 16-B
//                      loads, a workgroup histogram in LDS (1 KiB), one global atomic per non-zero bin at the end.
//   k_display_resolve  one workgroup: N = sum c[k], lo = N low / 100, hi = N high / 100, S = sum k |[cum_k, cum_k + c_k) n [lo, hi)|, C = hi - lo,
//                      q = 256 S / C, Lfix = ((q + 128) << 12) - (16 << 23) (the trimmed mean log2 Y in 23 fractional bits, at bin centres),
//                      e = bits(1) + (bits(key) - bits(1)) - Lfix clamped to [bits(min), bits(max)], E* = as_float(e): the inverse of the
//                      binning's log.  C == 0: E* = the previous exposure (1 without one).  E = E* without a previous exposure, else
//                      Eprev + (E* - Eprev) speed.  It writes the owner's record, the frame's own copy of E, a copy of the histogram, and
//                      clears the histogram for the next frame.
//   k_display_apply    one thread per pixel: v = lin E, the curve, out = sqrt(m) — the frame stays gamma-2 and k_present encodes it as before.

constexpr uint32_t kDisplayBins = 256;
constexpr uint32_t kDisplayPixelsPerThread = 4, kDisplayMaxGroups = 1024; // k_display_hist: at least 4 pixels per thread, at most 1024 workgroups

RFW_DI float display_luminance(const float4 c)
{
    const float r = c.x * c.x, g = c.y * c.y, b = c.z * c.z;
    float Y = 0.2126f * r;
    Y = Y + 0.7152f * g;
    Y = Y + 0.0722f * b;
    return Y;
}
// the bin of a luminance, or kDisplayBins: it does not count (NaN, zero, negative, below 2^-16)
RFW_DI uint32_t display_bin(const float Y)
{
    if (!(Y >= 0x1p-16f)) return kDisplayBins;
    const uint32_t b = (__float_as_uint(Y) >> 20) - 888u;
    return b < kDisplayBins - 1u ? b : kDisplayBins - 1u;
}

// Every lane adds 1 to its bin in LDS.  Measured against it and slower on the device (DESIGN.md "Display transform"): counting the lanes of a
// wavefront that share a bin with a ballot and adding once per distinct bin; four loads in flight per thread before the adds.
__global__ __launch_bounds__(256) void k_display_hist(const float4* __restrict__ frame, const uint64_t n, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_h[kDisplayBins];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t bin = display_bin(display_luminance(frame[i]));
        if (bin < kDisplayBins) atomicAdd(&s_h[bin], 1u);
    }
    __syncthreads();
    const uint32_t c = s_h[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

struct DisplayResolve {
    uint32_t low, high;          // percent, low < high
    uint32_t key_bits;           // bits(exposure_key)
    uint32_t min_bits, max_bits; // bits(exposure_min), bits(exposure_max)
    float speed;
    uint32_t has_prev;           // state[0] holds the exposure of the frame before
};

// state: (E applied, E*, q, N) of the owner; frame_e: this frame's own copy of E for k_display_apply (the next frame's resolve may overwrite
// the owner's record before this frame's apply has run, on another stream); hist_copy: the counts this frame resolved from
__global__ __launch_bounds__(256) void k_display_resolve(const DisplayResolve p, uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                          float* __restrict__ frame_e, uint32_t* __restrict__ hist_copy)
{
    __shared__ unsigned long long s_a[kDisplayBins];
    const uint32_t k = threadIdx.x;
    const uint32_t c = hist[k];
    hist[k] = 0u;
    hist_copy[k] = c;
    // inclusive prefix sum (Hillis-Steele: 8 steps of read, barrier, write, barrier)
    unsigned long long incl = c;
    s_a[k] = incl;
    __syncthreads();
    for (uint32_t d = 1u; d < kDisplayBins; d <<= 1) {
        const unsigned long long other = k >= d ? s_a[k - d] : 0ull;
        __syncthreads();
        incl += other;
        s_a[k] = incl;
        __syncthreads();
    }
    const unsigned long long N = s_a[kDisplayBins - 1u];
    const unsigned long long lo = (N * p.low) / 100ull, hi = (N * p.high) / 100ull;
    const unsigned long long cum = incl - c;
    const unsigned long long top = incl < hi ? incl : hi, bottom = cum > lo ? cum : lo;
    unsigned long long term = top > bottom ? (unsigned long long)k * (top - bottom) : 0ull;
    __syncthreads();
    s_a[k] = term;
    __syncthreads();
    for (uint32_t d = kDisplayBins / 2u; d > 0u; d >>= 1) {
        if (k < d) s_a[k] += s_a[k + d];
        __syncthreads();
    }
    if (k != 0u) return;
    const unsigned long long S = s_a[0], C = hi - lo;
    const float prev = __uint_as_float(state[0]);
    float target;
    uint32_t q = 0u;
    if (C == 0ull) {
        target = p.has_prev ? prev : 1.0f;
    } else {
        q = (uint32_t)((S * 256ull) / C);
        const int32_t Lfix = (int32_t)((q + 128u) << 12) - (16 << 23);
        const int32_t Kfix = (int32_t)p.key_bits - 0x3f800000;
        int32_t e = 0x3f800000 + Kfix - Lfix;
        if (e < (int32_t)p.min_bits) e = (int32_t)p.min_bits;
        if (e > (int32_t)p.max_bits) e = (int32_t)p.max_bits;
        target = __uint_as_float((uint32_t)e);
    }
    float E = target;
    if (p.has_prev) {
        float d = target - prev;
        d = d * p.speed;
        E = prev + d;
    }
    state[0] = __float_as_uint(E);
    state[1] = __float_as_uint(target);
    state[2] = q;
    state[3] = (uint32_t)N;
    *frame_e = E;
}

struct DisplayApply {
    uint32_t curve;  // 1 exposure only, 2 extended Reinhard, 3 ACES fit (Narkowicz)
    float white2;    // curve 2: W * W
    float exposure;  // used where frame_e is null (manual exposure)
};

RFW_DI float display_curve(const float lin, const float E, const DisplayApply p)
{
    const float v = lin * E;
    float m = v;
    if (p.curve == 2u) {
        float t = v / p.white2;
        t = 1.0f + t;
        const float n = v * t;
        const float dd = 1.0f + v;
        m = n / dd;
    } else if (p.curve == 3u) {
        float n = 2.51f * v;
        n = n + 0.03f;
        n = v * n;
        float dd = 2.43f * v;
        dd = dd + 0.59f;
        dd = v * dd;
        dd = dd + 0.14f;
        m = n / dd;
        if (m < 0.0f) m = 0.0f; // (compares: a NaN passes through)
        if (m > 1.0f) m = 1.0f;
    }
    return __builtin_sqrtf(m);
}

__global__ __launch_bounds__(256) void k_display_apply(const DisplayApply p, const float* __restrict__ frame_e, float4* __restrict__ frame, const uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float E = frame_e ? *frame_e : p.exposure;
    float4 c = frame[i];
    c.x = display_curve(c.x * c.x, E, p);
    c.y = display_curve(c.y * c.y, E, p);
    c.z = display_curve(c.z * c.z, E, p);
    frame[i] = c;
}

void launch_display_hist(hipStream_t s, const float4* frame, uint64_t n, uint32_t* hist)
{
    if (!n) return;
    const uint64_t want = (n + 256ull * kDisplayPixelsPerThread - 1ull) / (256ull * kDisplayPixelsPerThread);
    const dim3 grid((uint32_t)std::min<uint64_t>(want, kDisplayMaxGroups));
    hipLaunchKernelGGL(k_display_hist, grid, dim3(256), 0, s, frame, n, hist);
}
void launch_display_resolve(hipStream_t s, const DisplayParams& d, bool has_prev, uint32_t* hist, uint32_t* state, float* frame_e, uint32_t* hist_copy)
{
    DisplayResolve p;
    p.low = d.low; p.high = d.high;
    std::memcpy(&p.key_bits, &d.key, 4);
    std::memcpy(&p.min_bits, &d.exposure_min, 4);
    std::memcpy(&p.max_bits, &d.exposure_max, 4);
    p.speed = d.speed;
    p.has_prev = has_prev ? 1u : 0u;
    hipLaunchKernelGGL(k_display_resolve, dim3(1), dim3(256), 0, s, p, hist, state, frame_e, hist_copy);
}
void launch_display_apply(hipStream_t s, const DisplayParams& d, const float* frame_e, float4* frame, uint64_t n)
{
    if (!n) return;
    DisplayApply p;
    p.curve = d.curve;
    p.white2 = d.white * d.white;
    p.exposure = d.exposure;
    hipLaunchKernelGGL(k_display_apply, dim3((uint32_t)((n + 255ull) / 256ull)), dim3(256), 0, s, p, frame_e, frame, n);
}
