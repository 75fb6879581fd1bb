// overlay.inc — the 2D layer: the trait's 2D meshes (set_2d_mesh, set_2d_instances, render's view_2d) drawn over the finalised frame
// (DESIGN.md "2D layer"), included by kernels.hip inside namespace rfwhip.  Records and launch shape: kernels.h.
//
//   k_ov_setup   one thread per primitive (a triangle of a draw, in draw order): clip = view * (M * (v, 1)) in f32, the pixel position with
//                row 0 at the top, the snap to 8 sub-pixel bits; from there on integers: the doubled area S (a swap of vertices 1 and 2
//                makes it positive), the three edge functions, the top-left rule as the smallest value an edge function may take (0 or 1),
//                the box of pixels whose centre can be covered.  Dropped: w <= 0, not finite, |pixel| > 16384, S == 0, a texture that
//                does not exist.  No clipping: this is a 2D layer.
//   k_ov_bin     one wavefront per (bin of 64 x 64 pixels, 64 primitives): each lane tests one box against the bin; the ballot IS a word
//                of the bin's list: bit order is draw order, so nothing is compacted, counted or capped.
//   k_ov_raster  one workgroup per 16 x 16 pixels, a wavefront per 16 x 4, a pixel per lane.  The wavefront reads 64 words of its bin's list at
//                a time; of a word that is not zero each lane tests one primitive's box against the wavefront's pixels, and the ballot of
//                that is what the wavefront walks: the records it then reads are the same for every lane (uniform addresses: scalar
//                loads).  A lane keeps its pixel in registers: read at its first fragment, written once behind the last word, and only
//                if a fragment touched it.
//
// Edge i runs from vertex i to vertex i + 1; with y down and S > 0 the inside is where every E_i > 0.  An edge owns the pixels centred ON it
// when it is a top edge (dy == 0, dx > 0: the inside lies below it) or a left edge (dy < 0: it runs upwards, the inside lies to its right) —
// the neighbour across a shared edge walks it the other way round, so exactly one of the two draws such a pixel.
// Interpolation is affine in screen space: a = a_0 + l_1 (a_1 - a_0) + l_2 (a_2 - a_0) with l_1 = E_2 / S and l_2 = E_0 / S, f32 quotients of
// the exact integers — vertex 0 weighs what is left, so an attribute the three vertices share (opaque white text) is reproduced exactly.

constexpr float kOvMaxPixel = 16384.0f;

RFW_DI bool ov_finite(const float x) { return (fbits(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void k_ov_setup(const OvFrame f, const rfw_vertex_2d* __restrict__ vertices, const OvDraw* __restrict__ draws,
                                                  OvPrim* __restrict__ prims, OvTap* __restrict__ tap)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= f.n_prims) return;
    uint32_t lo = 0u, hi = f.n_draws; // the draw that holds draw position idx: the last one that starts at or before it
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (draws[mid].first_prim <= idx) lo = mid;
        else hi = mid;
    }
    const OvDraw& d = draws[lo];
    const uint32_t tri = idx - d.first_prim;
    const rfw_vertex_2d* const v = vertices + d.first_vertex + 3u * tri;
    const float* const M = d.m;
    const float* const V = f.view;
    float xp[3], yp[3];
    bool drop = false; // before the snap: a vertex without a pixel position
    for (int k = 0; k < 3; k++) {
        const float x = v[k].vertex[0], y = v[k].vertex[1], z = v[k].vertex[2];
        float q[4], c[4];
        for (int r = 0; r < 4; r++) q[r] = ((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r];
        for (int r = 0; r < 4; r++) c[r] = ((V[r] * q[0] + V[4 + r] * q[1]) + V[8 + r] * q[2]) + V[12 + r] * q[3];
        const float w = c[3];
        if (!ov_finite(c[0]) || !ov_finite(c[1]) || !ov_finite(c[2]) || !ov_finite(w) || !(w > 0.0f)) { drop = true; xp[k] = yp[k] = 0.0f; continue; }
        xp[k] = (c[0] / w * 0.5f + 0.5f) * (float)f.width;
        yp[k] = (0.5f - 0.5f * c[1] / w) * (float)f.height;
        if (!ov_finite(xp[k]) || !ov_finite(yp[k]) || gl_abs(xp[k]) > kOvMaxPixel || gl_abs(yp[k]) > kOvMaxPixel) { drop = true; xp[k] = yp[k] = 0.0f; }
    }
    int32_t X[3], Y[3];
    for (int k = 0; k < 3; k++) {
        X[k] = (int32_t)__builtin_rintf(xp[k] * 256.0f);
        Y[k] = (int32_t)__builtin_rintf(yp[k] * 256.0f);
    }
    OvTap t;
    for (int k = 0; k < 3; k++) { t.X[k] = drop ? 0 : X[k]; t.Y[k] = drop ? 0 : Y[k]; }
    if (d.tex >= 0 && (uint32_t)d.tex >= f.n_textures) drop = true; // a texture that does not exist (the tap keeps the snapped vertices)
    t.mesh = d.mesh; t.instance = d.instance; t.triangle = tri;
    t.pad[0] = t.pad[1] = 0u;

    int64_t S = (int64_t)(X[1] - X[0]) * (int64_t)(Y[2] - Y[0]) - (int64_t)(Y[1] - Y[0]) * (int64_t)(X[2] - X[0]);
    if (S == 0) drop = true;
    t.dropped = drop ? 1u : 0u;
    tap[idx] = t;

    int order[3] = {0, 1, 2};
    if (S < 0) { order[1] = 2; order[2] = 1; S = -S; }
    OvPrim p;
    p.S = S;
    p.tex = d.tex;
    int32_t minx = X[0], maxx = X[0], miny = Y[0], maxy = Y[0];
    for (int i = 0; i < 3; i++) {
        const int a = order[i], b = order[(i + 1) % 3];
        const int32_t dx = X[b] - X[a], dy = Y[b] - Y[a];
        p.A[i] = -dy;
        p.B[i] = dx;
        p.C[i] = (int64_t)(-dy) * (int64_t)(128 - X[a]) + (int64_t)dx * (int64_t)(128 - Y[a]);
        p.need[i] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
        minx = X[a] < minx ? X[a] : minx; maxx = X[a] > maxx ? X[a] : maxx;
        miny = Y[a] < miny ? Y[a] : miny; maxy = Y[a] > maxy ? Y[a] : maxy;
        p.uv[i][0] = v[a].uv[0]; p.uv[i][1] = v[a].uv[1];
        for (int c = 0; c < 4; c++) p.color[i][c] = v[a].color[c];
    }
    // pixels whose centre 256 p + 128 lies in [min, max] (arithmetic shifts: floor for negative values too), clipped to the frame
    int32_t x0 = (minx - 128 + 255) >> 8, x1 = (maxx - 128) >> 8, y0 = (miny - 128 + 255) >> 8, y1 = (maxy - 128) >> 8;
    x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
    x1 = x1 > (int32_t)f.width - 1 ? (int32_t)f.width - 1 : x1;
    y1 = y1 > (int32_t)f.height - 1 ? (int32_t)f.height - 1 : y1;
    if (drop || y0 > y1) { x0 = 1; x1 = 0; y0 = 1; y1 = 0; }
    p.x0 = x0; p.y0 = y0; p.x1 = x1; p.y1 = y1;
    prims[idx] = p;
}

__global__ __launch_bounds__(256) void k_ov_bin(const OvFrame f, const OvPrim* __restrict__ prims, uint64_t* __restrict__ words)
{
    // one wavefront per (bin, word): the words of a bin are independent of one another, so nothing walks them in sequence
    const uint32_t bin = blockIdx.x, lane = threadIdx.x & 63u, c = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (c >= f.chunks) return;
    const int32_t bx0 = (int32_t)((bin % f.bins_x) * kOvBin), by0 = (int32_t)((bin / f.bins_x) * kOvBin);
    const int32_t bx1 = bx0 + (int32_t)kOvBin - 1, by1 = by0 + (int32_t)kOvBin - 1;
    const uint32_t i = c * 64u + lane;
    bool touches = false;
    if (i < f.n_prims) {
        const OvPrim& p = prims[i];
        const int32_t x0 = p.x0, y0 = p.y0, x1 = p.x1, y1 = p.y1;
        touches = x0 <= x1 && x0 <= bx1 && x1 >= bx0 && y0 <= by1 && y1 >= by0;
    }
    const unsigned long long m = __ballot(touches);
    if (lane == 0u) words[(size_t)bin * f.chunks + c] = m;
}

__global__ __launch_bounds__(256) void k_ov_raster(const OvFrame f, const OvPrim* __restrict__ prims, const uint64_t* __restrict__ words,
                                                   const uint32_t* __restrict__ tex_data, const TexDesc* __restrict__ tex_desc, float4* __restrict__ frame)
{
    const int32_t wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    const int32_t wx0 = (int32_t)(blockIdx.x * kOvTile), wy0 = (int32_t)(blockIdx.y * kOvTile) + 4 * wave; // the wavefront's 16 x 4 pixels
    const int32_t wx1 = wx0 + 15, wy1 = wy0 + 3;
    const int32_t px = wx0 + (int32_t)(lane & 15u), py = wy0 + (int32_t)(lane >> 4);
    const bool in_frame = px < (int32_t)f.width && py < (int32_t)f.height;
    const uint32_t bin = (blockIdx.y / (kOvBin / kOvTile)) * f.bins_x + blockIdx.x / (kOvBin / kOvTile);
    const uint64_t* const list = words + (size_t)bin * f.chunks;
    const size_t at = (size_t)(in_frame ? py : 0) * f.width + (size_t)(in_frame ? px : 0);
    float4 dst = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool loaded = false, touched = false;
    // 64 words of the bin's list per step, one per lane; the words that are not zero are then taken in order.  Of such a word's primitives
    // every lane tests ONE box against the wavefront's 16 x 4 pixels: the ballot of that is the list the wavefront walks, still in draw order.
    for (uint32_t base = 0; base < f.chunks; base += 64u) {
        const unsigned long long mine = base + lane < f.chunks ? list[base + lane] : 0ull;
        unsigned long long live = __ballot(mine != 0ull);
        while (live) {
            const int wl = __builtin_ctzll(live);
            live &= live - 1ull;
            const uint32_t c = base + (uint32_t)wl;
            const unsigned long long word = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), wl) << 32) |
                                            (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, wl);
            bool near = false;
            if ((word >> lane) & 1ull) {
                const OvPrim& q = prims[(size_t)c * 64u + lane];
                near = !(q.x0 > wx1 || q.x1 < wx0 || q.y0 > wy1 || q.y1 < wy0);
            }
            unsigned long long m = __ballot(near);
            while (m) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(m);
                m &= m - 1ull;
                const OvPrim& p = prims[(size_t)c * 64u + bit];
                if (!in_frame) continue;
                const int64_t E0 = p.C[0] + ((int64_t)p.A[0] * px + (int64_t)p.B[0] * py) * 256;
                const int64_t E1 = p.C[1] + ((int64_t)p.A[1] * px + (int64_t)p.B[1] * py) * 256;
                const int64_t E2 = p.C[2] + ((int64_t)p.A[2] * px + (int64_t)p.B[2] * py) * 256;
                if (E0 < (int64_t)p.need[0] || E1 < (int64_t)p.need[1] || E2 < (int64_t)p.need[2]) continue;
                const float s = (float)p.S;
                // (the weight of vertex 0 is 1 - l1 - l2: written so that an attribute the three vertices share comes out exactly)
                const float l1 = (float)E2 / s, l2 = (float)E0 / s;
                float src[4];
                for (int k = 0; k < 4; k++) src[k] = (p.color[0][k] + l1 * (p.color[1][k] - p.color[0][k])) + l2 * (p.color[2][k] - p.color[0][k]);
                if (p.tex >= 0) {
                    const float u = (p.uv[0][0] + l1 * (p.uv[1][0] - p.uv[0][0])) + l2 * (p.uv[2][0] - p.uv[0][0]);
                    const float v = (p.uv[0][1] + l1 * (p.uv[1][1] - p.uv[0][1])) + l2 * (p.uv[2][1] - p.uv[0][1]);
                    const f4 t = texture_sample(tex_data, tex_desc[p.tex], u, v, 0.0f);
                    src[0] = src[0] * t.x; src[1] = src[1] * t.y; src[2] = src[2] * t.z; src[3] = src[3] * t.w;
                }
                const float a = src[3];
                if (!ov_finite(a) || !(a > 0.0f)) continue; // the reference's discard
                if (!loaded) { dst = frame[at]; loaded = true; }
                touched = true;
                if (a >= 1.0f) { dst.x = src[0]; dst.y = src[1]; dst.z = src[2]; }
                else {
                    const float ia = 1.0f - a;
                    dst.x = a * src[0] + ia * dst.x;
                    dst.y = a * src[1] + ia * dst.y;
                    dst.z = a * src[2] + ia * dst.z;
                }
            }
        }
    }
    if (touched) frame[at] = dst;
}

void launch_overlay(hipStream_t s, const OvFrame& f, const rfw_vertex_2d* vertices, const OvDraw* draws, OvPrim* prims, OvTap* tap, uint64_t* words,
                    const uint32_t* tex_data, const TexDesc* tex_desc, float4* frame)
{
    if (f.n_prims == 0u || f.width == 0u || f.height == 0u) return;
    hipLaunchKernelGGL(k_ov_setup, dim3((f.n_prims + 255u) / 256u), dim3(256), 0, s, f, vertices, draws, prims, tap);
    hipLaunchKernelGGL(k_ov_bin, dim3(f.bins_x * f.bins_y, (f.chunks + 3u) / 4u), dim3(256), 0, s, f, prims, words);
    const dim3 grid((f.width + kOvTile - 1u) / kOvTile, (f.height + kOvTile - 1u) / kOvTile);
    hipLaunchKernelGGL(k_ov_raster, grid, dim3(256), 0, s, f, prims, words, tex_data, tex_desc, frame);
}
