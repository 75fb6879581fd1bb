// denoise.inc — option "denoise" (include/rfw_hip.h, DESIGN.md "Denoiser"): an edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) of
// the albedo-demodulated radiance of the path-traced frame, guided by the primary hit, in place of k_assemble.  Included by kernels.hip inside
// namespace rfwhip, after aov.inc (primary_surface) and finalise<>.
//
//   k_dn_guide  after k_primary at bounce 0, before k_shade: per frame pixel three float4 planes, g0 = (faced gN, t), g1 = (P, 0),
//               g2 = (albedo, f); f = 1 where the pixel is filtered (the camera ray hit something that is not a light), else 0
//   k_atrous    pass i of k, step s = 2^i: x_{i+1}(p) = sum_q w(p, q) x_i(q) / sum_q w(p, q) over the 5 x 5 taps q = p + s (dx, dy) inside the
//               frame with f(q) = 1.  The first pass reads the accumulator slab and demodulates (x_0 = (acc / n) / max(albedo, kDnAlbedoFloor)),
//               the last one remodulates, takes k_assemble's square root and writes the frame; pixels with f = 0 pass through with k_assemble's
//               finalise.  Between passes x travels in float4 planes whose w holds f.
//   k_dn_temporal  option "denoise_temporal" (DESIGN.md "Denoiser: temporal"), between the trace and the passes: x_0 of this image blended with
//               the previous image's x_0, fetched where this pixel's primary hit lay in the previous view and weighted by the a-trous normal
//               and plane weights; the result (x.rgb, h) and the frame's (g0, g1) are the history the next image reads.  The passes then start
//               from that plane as passes after the first do (h > 0 exactly where f = 1 and x is finite).
//   k_dn_ids, k_dn_motion, k_dn_temporal_motion  option "denoise_motion" (DESIGN.md "Denoiser: motion"): the instance id of every pixel's primary
//               hit, one record per instance that carries a point and a normal of this image into the instance's pose of the previous image,
//               and k_dn_temporal reprojecting through that record, its taps restricted to the same instance.
//   k_dn_tris, k_dn_pose, k_dn_temporal_deform  option "denoise_deform" (DESIGN.md "Denoiser: deforming meshes"): the triangle and barycentrics of
//               every pixel's primary hit, a snapshot of the mesh-space vertices of every skinned copy that travels with the history, and
//               k_dn_temporal reprojecting a skinned copy's pixel through the pose its triangle had in the previous image.
//
// Two forms of a pass.  DIRECT: one thread per pixel, 25 taps straight from memory.  TILED: for step s the pixels with equal (x mod s, y mod s)
// form s^2 sub-images on each of which the pass is a dense 5 x 5 filter; a workgroup takes 16 x 16 pixels of ONE sub-image and stages their
// 20 x 20 window of (x, g0, g1) in LDS once.  LDS rows are kDnPitch = 32 float4 apart: a ds_read_b128 is served in groups of 16 lanes that span
// two rows of the tile (lanes 0-3, 12-15 of one row with lanes 4-11 of the next), and those hit 16 different 16-byte slots of the 256-byte bank
// row only when the pitch is a multiple of 16 slots.

constexpr float kDnPlane = 0.02f;       // wp = max(0, 1 - |dot(gN_p, P_q - P_p)| / (kDnPlane t_p)): distance from p's tangent plane, relative to the viewing distance
constexpr int kDnNormalSquarings = 5;   // wn = max(0, dot(gN_p, gN_q))^32
constexpr float kDnAlbedoFloor = 1e-3f; // demodulation divides by max(albedo, this) per channel
constexpr float kDnTemporalMinWeight = 0.25f; // a reprojected pixel keeps its history while the weights of its four taps sum to this (of at most 1)
constexpr int kDnTile = 16, kDnRadius = 2, kDnSpan = kDnTile + 2 * kDnRadius, kDnPitch = 32;
constexpr float kDnH[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
// which form pass i (step 2^i) takes unless option "denoise_form" forces one.  Timed per step at 1080p on the MI355X (EXPERIMENTS.md, "denoiser"):
// tiled 0.16 / 0.10 / 0.13 / 0.21 / 0.16 ms for steps 1 .. 16 against direct 0.57 / 0.22 / 0.17 / 0.20 / 0.30 — tiled everywhere (step 8 is a tie)
constexpr bool atrous_tiled_by_default(uint32_t /*pass*/) { return true; }

struct DnParams {
    const float4* acc;    // the instance's accumulator slab(s), as k_assemble reads them
    uint64_t slab_elems;
    const float4* guide;  // g0, g1, g2: three planes of width x height
    const float4* in;     // x_i (rgb, f): passes after the first
    float4* out;          // x_{i+1} (rgb, f), or the frame (last pass)
    uint32_t samples;     // n, the sample just traced included
    uint32_t step_shift;  // s = 1 << step_shift
    float inv_sigma2;     // 1 / sigma_i^2, sigma_i = sigma_c 2^-i / sqrt(n)
};

__global__ __launch_bounds__(256) void k_dn_guide(const CameraParams cam, const SceneDev sc, const PathDev p, float4* __restrict__ guide, const uint32_t pixel_mask)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= p.capacity) return;
    const uint4 S = p.hit[0][idx];
    if (S.x == kNoPath) return; // a slab slot without a pixel
    const float4 O4 = p.ray_o[0][idx], D4 = p.ray_d[0][idx];
    const uint32_t px = fbits(O4.w) & pixel_mask; // (a batch of samples carries the sample's index above the pixel's)
    const uint32_t plane = cam.width * cam.height;
    if (px >= plane) return;
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, g2 = g0;
    if ((int32_t)S.x >= 0) {
        const PrimarySurface ps = primary_surface(cam, sc, S, O4, D4);
        g0 = make_float4(ps.gN.x, ps.gN.y, ps.gN.z, ps.t);
        g1 = make_float4(ps.P.x, ps.P.y, ps.P.z, 0.0f);
        g2 = make_float4(ps.albedo.x, ps.albedo.y, ps.albedo.z, ps.light ? 0.0f : 1.0f);
    }
    guide[px] = g0;
    guide[(size_t)plane + px] = g1;
    guide[2u * (size_t)plane + px] = g2;
}

struct DnPixel { float4 x, g0, g1; }; // x.w = f; g0, g1 are read only where f = 1

template <bool FIRST> RFW_DI DnPixel dn_load(const CameraParams& cam, const DnParams& dp, const int x, const int y)
{
    DnPixel r;
    r.x = r.g0 = r.g1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // outside the frame, or not filtered: weight 0
    if (x < 0 || y < 0 || x >= (int)cam.width || y >= (int)cam.height) return r;
    const uint32_t i = (uint32_t)x + (uint32_t)y * cam.width;
    const size_t plane = (size_t)cam.width * cam.height;
    if (FIRST) {
        const float4 g2 = dp.guide[2u * plane + i];
        if (!(g2.w > 0.0f)) return r;
        uint32_t owner;
        const uint32_t slot = pixel_to_slab(cam, (uint32_t)x, (uint32_t)y, owner);
        const float4 a = dp.acc[(uint64_t)owner * dp.slab_elems + slot];
        const float n = (float)(int)dp.samples;
        r.x = make_float4((a.x * 1.0f / n) / gl_max(g2.x, kDnAlbedoFloor), (a.y * 1.0f / n) / gl_max(g2.y, kDnAlbedoFloor),
                          (a.z * 1.0f / n) / gl_max(g2.z, kDnAlbedoFloor), 1.0f);
    } else {
        r.x = dp.in[i];
        if (!(r.x.w > 0.0f)) return r;
    }
    r.g0 = dp.guide[i];
    r.g1 = dp.guide[plane + i];
    return r;
}

// sw += w(p, q), sx += w(p, q) x(q); inv_plane = 1 / (kDnPlane t_p)
RFW_DI void dn_tap(const DnPixel& p, const float inv_plane, const float inv_sigma2, const float h, const float4 xq, const float4 g0q, const float4 g1q, float& sw,
                   f3& sx)
{
    if (!(xq.w > 0.0f)) return;
    float wn = gl_max(0.0f, p.g0.x * g0q.x + p.g0.y * g0q.y + p.g0.z * g0q.z);
    for (int k = 0; k < kDnNormalSquarings; k++) wn = wn * wn;
    const float d = p.g0.x * (g1q.x - p.g1.x) + p.g0.y * (g1q.y - p.g1.y) + p.g0.z * (g1q.z - p.g1.z);
    const float wp = gl_max(0.0f, 1.0f - gl_abs(d) * inv_plane);
    const float cx = p.x.x - xq.x, cy = p.x.y - xq.y, cz = p.x.z - xq.z;
    const float d2 = cx * cx + cy * cy + cz * cz;
    if (!(d2 < 3.0e38f)) return; // a tap that is not finite (a NaN or Inf accumulator pixel) stays where it is: it spoils its own pixel only
    const float wc = rfw_expf(-(d2 * inv_sigma2));
    const float w = h * wn * wp * wc;
    sw += w;
    sx = sx + w * mk3(xq.x, xq.y, xq.z);
}

template <bool FIRST, bool LAST, bool TILED>
__global__ __launch_bounds__(kDnTile * kDnTile) void k_atrous(const CameraParams cam, const DnParams dp)
{
    const int shift = (int)dp.step_shift, s = 1 << shift;
    const int lx = (int)(threadIdx.x % kDnTile), ly = (int)(threadIdx.x / kDnTile);
    int px, py;
    DnPixel c;
    float sw = 0.0f;
    f3 sx = mk3(0.0f);
    if (TILED) {
        __shared__ float4 s_x[kDnSpan * kDnPitch], s_g0[kDnSpan * kDnPitch], s_g1[kDnSpan * kDnPitch];
        // sub-image (ox, oy) of the step, and the window's first pixel in sub-image coordinates
        const int ox = (int)blockIdx.x & (s - 1), oy = (int)blockIdx.y & (s - 1);
        const int i0 = (int)(blockIdx.x >> shift) * kDnTile - kDnRadius, j0 = (int)(blockIdx.y >> shift) * kDnTile - kDnRadius;
        for (int k = (int)threadIdx.x; k < kDnSpan * kDnSpan; k += kDnTile * kDnTile) {
            const int wx = k % kDnSpan, wy = k / kDnSpan;
            const DnPixel q = dn_load<FIRST>(cam, dp, ox + (i0 + wx) * s, oy + (j0 + wy) * s); // (left of / above the frame: negative)
            s_x[wy * kDnPitch + wx] = q.x;
            s_g0[wy * kDnPitch + wx] = q.g0;
            s_g1[wy * kDnPitch + wx] = q.g1;
        }
        __syncthreads();
        px = ox + (i0 + kDnRadius + lx) * s;
        py = oy + (j0 + kDnRadius + ly) * s;
        if (px >= (int)cam.width || py >= (int)cam.height) return;
        const int at = (ly + kDnRadius) * kDnPitch + lx + kDnRadius;
        c.x = s_x[at]; c.g0 = s_g0[at]; c.g1 = s_g1[at];
        if (c.x.w > 0.0f) {
            const float inv_plane = 1.0f / (kDnPlane * c.g0.w);
#pragma unroll
            for (int dy = 0; dy <= 2 * kDnRadius; dy++)
#pragma unroll
                for (int dx = 0; dx <= 2 * kDnRadius; dx++) {
                    const int k = (ly + dy) * kDnPitch + lx + dx;
                    dn_tap(c, inv_plane, dp.inv_sigma2, kDnH[dx] * kDnH[dy], s_x[k], s_g0[k], s_g1[k], sw, sx);
                }
        }
    } else {
        px = (int)(blockIdx.x * kDnTile) + lx;
        py = (int)(blockIdx.y * kDnTile) + ly;
        if (px >= (int)cam.width || py >= (int)cam.height) return;
        c = dn_load<FIRST>(cam, dp, px, py);
        if (c.x.w > 0.0f) {
            const float inv_plane = 1.0f / (kDnPlane * c.g0.w);
            for (int dy = 0; dy <= 2 * kDnRadius; dy++)
                for (int dx = 0; dx <= 2 * kDnRadius; dx++) {
                    const DnPixel q = dn_load<FIRST>(cam, dp, px + (dx - kDnRadius) * s, py + (dy - kDnRadius) * s);
                    dn_tap(c, inv_plane, dp.inv_sigma2, kDnH[dx] * kDnH[dy], q.x, q.g0, q.g1, sw, sx);
                }
        }
    }
    const bool filtered = c.x.w > 0.0f; // (then sw >= h(0)^2 wn(p, p) > 0: the centre tap — unless x(p) itself is not finite: 0 / 0, the pixel stays bad)
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (filtered) out = make_float4(sx.x / sw, sx.y / sw, sx.z / sw, 1.0f);
    const uint32_t i = (uint32_t)px + (uint32_t)py * cam.width;
    if (LAST) {
        uint32_t owner;
        const uint32_t slot = pixel_to_slab(cam, (uint32_t)px, (uint32_t)py, owner);
        const float4 a = dp.acc[(uint64_t)owner * dp.slab_elems + slot];
        const float n = (float)(int)dp.samples;
        if (filtered) {
            const float4 g2 = dp.guide[2u * (size_t)cam.width * cam.height + i];
            out.x = __builtin_sqrtf(out.x * gl_max(g2.x, kDnAlbedoFloor));
            out.y = __builtin_sqrtf(out.y * gl_max(g2.y, kDnAlbedoFloor));
            out.z = __builtin_sqrtf(out.z * gl_max(g2.z, kDnAlbedoFloor));
        } else {
            out.x = finalise<false>(a.x, n);
            out.y = finalise<false>(a.y, n);
            out.z = finalise<false>(a.z, n);
        }
        out.w = finalise<false>(a.w, n);
    }
    dp.out[i] = out;
}

// One history: three planes of width x height, (x.rgb, h), g0 = (gN, t) and g1 = (P, 0) of the frame that wrote it; h = samples behind x, 0 = none
struct DnTemporalParams {
    const float4* acc;    // as DnParams
    uint64_t slab_elems;
    const float4* guide;  // this frame's g0, g1, g2
    const float4* prev;   // the previous image's history, or null: there is none
    float4* cur;          // this image's
    float pos[3], p1[3], right[3], up[3]; // the view of the frame that wrote prev
    uint32_t samples;     // n, the sample just traced included
    float max_history;    // Hmax
};

constexpr uint32_t kDnNoId = 0xffffffffu; // id planes: the camera ray missed

// option "denoise_motion".  Per frame pixel the instance id of the primary hit, next to k_dn_guide and with its bounds handling.
__global__ __launch_bounds__(256) void k_dn_ids(const CameraParams cam, const PathDev p, uint32_t* __restrict__ ids, const uint32_t pixel_mask)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= p.capacity) return;
    const uint4 S = p.hit[0][idx];
    if (S.x == kNoPath) return; // a slab slot without a pixel
    const uint32_t px = fbits(p.ray_o[0][idx].w) & pixel_mask;
    if (px >= cam.width * cam.height) return;
    ids[px] = (int32_t)S.x >= 0 ? S.x : kDnNoId;
}

// option "denoise_deform".  Per frame pixel the triangle of the primary hit, next to k_dn_ids and with its bounds handling: x = the row of the
// device triangle buffer (hit[0].y) with bit 31 set iff primary_surface negates the geometric normal, y = the packed barycentrics (hit[0].w)
constexpr uint32_t kDnFlipped = 0x80000000u;
__global__ __launch_bounds__(256) void k_dn_tris(const CameraParams cam, const SceneDev sc, const PathDev p, uint2* __restrict__ tris, const uint32_t pixel_mask)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= p.capacity) return;
    const uint4 S = p.hit[0][idx];
    if (S.x == kNoPath) return; // a slab slot without a pixel
    const uint32_t px = fbits(p.ray_o[0][idx].w) & pixel_mask;
    if (px >= cam.width * cam.height) return;
    uint2 out = make_uint2(kDnNoId, 0u);
    if ((int32_t)S.x >= 0) {
        const float4 D4 = p.ray_d[0][idx];
        const float4 q3 = reinterpret_cast<const float4*>(sc.triangles + S.y)[3];
        const float4* np = reinterpret_cast<const float4*>(sc.instance_normals + (int32_t)S.x);
        const f3 gN = normalize(xform_rows(np[0], np[1], np[2], mk3(q3.x, q3.y, q3.z), 0.0f)); // primary_surface's, step for step
        out = make_uint2(S.y | (dot(mk3(D4.x, D4.y, D4.z), gN) >= 0.0f ? kDnFlipped : 0u), S.w);
    }
    tris[px] = out;
}

// One skinned copy of a frame: (first row of the triangle buffer, triangles, first triangle of the pose snapshot, mesh record index); in the
// table the host builds the copies stand in snapshot order.  Per instance id of a frame (DnCopyRef, next to the snapshot): the first three
// words of its copy, (0, 0, 0, 0) where the instance is no skinned copy.
typedef uint4 DnCopy;
typedef uint4 DnCopyRef;

// The pose snapshot of a history: tp[0..3] of every triangle of every skinned copy (the mesh-space vertices with their w words, the stored
// geometric normal).  One thread per float4, all copies in one launch.
__global__ __launch_bounds__(256) void k_dn_pose(const rfw_rt_triangle* __restrict__ triangles, const DnCopy* __restrict__ copies, const uint32_t n_copies,
                                                 const uint32_t total, float4* __restrict__ out)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (n_copies == 0u || (t >> 2) >= total) return;
    const uint32_t tri = t >> 2;
    uint32_t lo = 0u, hi = n_copies; // the last copy that starts at or before tri
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (copies[mid].z <= tri) lo = mid;
        else hi = mid;
    }
    const DnCopy c = copies[lo];
    const uint32_t local = tri - c.z;
    if (local >= c.y) return;
    out[t] = reinterpret_cast<const float4*>(triangles + c.x + local)[t & 3u];
}

// What a history keeps of every instance of the frame that wrote it, and what k_dn_motion makes of two of them
struct alignas(16) DnInstance {
    float m[16];       // the forward matrix M, column major (rfw_mat4)
    float n[3][4];     // InstanceNormal: the rows of transpose(inverse(M))
    uint32_t mesh, valid, pad[2]; // InstanceXform::mesh, flags & 1
};
static_assert(sizeof(DnInstance) == kDnInstanceBytes, "DnInstance");
struct alignas(16) DnMotion {
    float a[3][4];     // rows of A = M' inverse(M): a point of this image -> where the instance held it in the previous image
    float b[3][4];     // rows of B = N' transpose(M) = transpose(inverse(A)) in [0..2]; [0][3] holds the state's bits, [1][3] = [2][3] = 0
};
static_assert(sizeof(DnMotion) == kDnMotionBytes, "DnMotion");

// One thread per instance of this frame: its record, and its entry of the snapshot that travels with the history this image writes.
// state 0 = no history (a new, removed or re-meshed instance, a matrix that is not affine, a record that is not finite), 1 = the matrix is the
// previous image's bit for bit, 2 = moved.  Plain float32, every sum left to right.
// Option "denoise_deform" (cur_refs != null): the instance's DnCopyRef, and state 3 = deforming — a skinned copy in both images, of the same
// mesh record and triangle count: the record then holds the rows of the previous forward matrix M' in a and of the previous InstanceNormal
// in b, for k_dn_temporal_deform to carry the previous pose of the pixel's triangle into the previous image's world.
__global__ __launch_bounds__(64) void k_dn_motion(const rfw_mat4* __restrict__ matrices, const InstanceXform* __restrict__ xf, const InstanceNormal* __restrict__ nm,
                                                  const uint32_t n, const DnInstance* __restrict__ prev, const uint32_t n_prev, DnInstance* __restrict__ cur,
                                                  DnMotion* __restrict__ out, const DnCopy* __restrict__ copies, const uint32_t n_copies,
                                                  const DnCopyRef* __restrict__ prev_refs, DnCopyRef* __restrict__ cur_refs)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    DnInstance c;
    for (int k = 0; k < 16; k++) c.m[k] = matrices[i].m[k];
    const InstanceXform x = xf[i];
    const InstanceNormal nn = nm[i];
    for (int k = 0; k < 4; k++) { c.n[0][k] = nn.n_r0[k]; c.n[1][k] = nn.n_r1[k]; c.n[2][k] = nn.n_r2[k]; }
    c.mesh = x.mesh;
    c.valid = x.flags & 1u;
    c.pad[0] = c.pad[1] = 0u;
    cur[i] = c;
    DnCopyRef ref = make_uint4(0u, 0u, 0u, 0u);
    if (cur_refs != nullptr) {
        if (c.valid != 0u)
            for (uint32_t k = 0; k < n_copies; k++) {
                const DnCopy cp = copies[k];
                if (cp.w == c.mesh) ref = make_uint4(cp.x, cp.y, cp.z, 0u);
            }
        cur_refs[i] = ref;
    }
    DnMotion r;
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 4; k++) r.a[j][k] = r.b[j][k] = 0.0f;
    uint32_t state = 0u;
    if (prev != nullptr && i < n_prev) {
        const DnInstance q = prev[i];
        const auto affine = [](const float* m) { return fbits(m[3]) == 0u && fbits(m[7]) == 0u && fbits(m[11]) == 0u && fbits(m[15]) == 0x3f800000u; };
        const bool linked = q.valid != 0u && c.valid != 0u && q.mesh == c.mesh && affine(q.m) && affine(c.m);
        const bool deforming = cur_refs != nullptr && prev_refs != nullptr && ref.y != 0u && prev_refs[i].y == ref.y;
        if (linked && deforming) { // the previous matrix and normal rows as they are: the temporal kernel applies them to the previous pose
            bool finite = true;
            for (int j = 0; j < 3; j++) {
                for (int k = 0; k < 4; k++) {
                    r.a[j][k] = q.m[4 * k + j];
                    finite = finite && gl_abs(r.a[j][k]) <= 3.0e38f;
                }
                for (int k = 0; k < 3; k++) {
                    r.b[j][k] = q.n[j][k];
                    finite = finite && gl_abs(r.b[j][k]) <= 3.0e38f;
                }
            }
            state = finite ? 3u : 0u;
        } else if (linked) {
            bool same = true;
            for (int k = 0; k < 16; k++) same = same && fbits(q.m[k]) == fbits(c.m[k]);
            const float* inv[3] = {x.inv_r0, x.inv_r1, x.inv_r2}; // row k of inverse(M); its fourth row is (0, 0, 0, 1)
            bool finite = true;
            for (int j = 0; j < 3; j++) {
                for (int k = 0; k < 4; k++) { // row j of M' = (m'[j], m'[4 + j], m'[8 + j], m'[12 + j])
                    float s = (q.m[j] * inv[0][k] + q.m[4 + j] * inv[1][k]) + q.m[8 + j] * inv[2][k];
                    if (k == 3) s = s + q.m[12 + j];
                    r.a[j][k] = s;
                    finite = finite && gl_abs(s) <= 3.0e38f;
                }
                for (int k = 0; k < 3; k++) { // transpose(M)[l][k] = M[k][l] = m[4 l + k]
                    const float s = (q.n[j][0] * c.m[k] + q.n[j][1] * c.m[4 + k]) + q.n[j][2] * c.m[8 + k];
                    r.b[j][k] = s;
                    finite = finite && gl_abs(s) <= 3.0e38f;
                }
            }
            state = !finite ? 0u : same ? 1u : 2u;
        }
    }
    r.b[0][3] = bitsf(state);
    out[i] = r;
}

struct DnDeformParams {
    const uint2* tris;          // this frame's triangle plane (k_dn_tris)
    const DnCopyRef* refs;      // one per instance id of this frame
    const DnCopyRef* prev_refs; // ... and of the frame that wrote tp.prev; read only for ids whose state is 3
    const float4* prev_pose;    // that frame's pose snapshot, four float4 per triangle
};

struct DnMotionParams {
    const uint32_t* ids;      // this frame's instance ids
    const uint32_t* prev_ids; // those of the frame that wrote tp.prev (null with it)
    uint32_t* cur_ids;        // ... and that travel with tp.cur
    const DnMotion* records;  // one per instance id of this frame
    uint32_t n_records;
};

// k_dn_temporal and, with MOTION, k_dn_temporal_motion: there the hit (P, gN) is first carried into the previous image's pose of its instance
// (state 2), a tap must show the same instance, and an instance without a record there (state 0) has no history.  With DEFORM,
// k_dn_temporal_deform: a pixel of a deforming instance (state 3) takes P and gN from its triangle's vertices in the previous image's pose
// snapshot, at the hit's barycentrics, under the previous instance matrix; from there on it is a state 2 pixel.
template <bool MOTION, bool DEFORM> RFW_DI void dn_temporal_pixel(const CameraParams& cam, const DnTemporalParams& tp, const DnMotionParams& mp, const DnDeformParams& df)
{
    const int px = (int)(blockIdx.x * kDnTile + threadIdx.x % kDnTile), py = (int)(blockIdx.y * kDnTile + threadIdx.x / kDnTile);
    if (px >= (int)cam.width || py >= (int)cam.height) return;
    const int W = (int)cam.width, H = (int)cam.height;
    const size_t plane = (size_t)cam.width * cam.height;
    const uint32_t i = (uint32_t)px + (uint32_t)py * cam.width;
    const float4 g0 = tp.guide[i], g1 = tp.guide[plane + i], g2 = tp.guide[2u * plane + i];
    tp.cur[plane + i] = g0;
    tp.cur[2u * plane + i] = g1;
    uint32_t id = kDnNoId;
    if (MOTION) {
        id = mp.ids[i];
        mp.cur_ids[i] = id;
    }
    if (!(g2.w > 0.0f)) {
        tp.cur[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    uint32_t owner;
    const uint32_t slot = pixel_to_slab(cam, (uint32_t)px, (uint32_t)py, owner);
    const float4 a = tp.acc[(uint64_t)owner * tp.slab_elems + slot];
    const float n = (float)(int)tp.samples;
    const f3 c = mk3((a.x * 1.0f / n) / gl_max(g2.x, kDnAlbedoFloor), (a.y * 1.0f / n) / gl_max(g2.y, kDnAlbedoFloor), (a.z * 1.0f / n) / gl_max(g2.z, kDnAlbedoFloor));
    f3 x = c;
    float hh = 0.0f;
    f3 P = mk3(g1.x, g1.y, g1.z), N = mk3(g0.x, g0.y, g0.z);
    bool history = tp.prev != nullptr;
    if (MOTION && history) {
        uint32_t state = 0u;
        if (id < mp.n_records) { // (neighbouring pixels share an instance: a cached vector load, not uniform across the wavefront)
            const float4* rp = reinterpret_cast<const float4*>(mp.records + id);
            const float4 b0 = rp[3];
            state = fbits(b0.w);
            if (state == 2u) {
                const float4 a0 = rp[0], a1 = rp[1], a2 = rp[2], b1 = rp[4], b2 = rp[5];
                N = normalize(xform_rows(b0, b1, b2, N, 0.0f));
                P = xform_rows(a0, a1, a2, P, 1.0f);
            }
            if (DEFORM && state == 3u) { // the pixel's triangle in the pose and under the matrix of the previous image
                const uint2 tr = df.tris[i];
                const DnCopyRef cr = df.refs[id], pr = df.prev_refs[id];
                const uint32_t local = (tr.x & ~kDnFlipped) - cr.x;
                state = 0u;
                if (local < pr.y) { // (a row outside the copy: no history)
                    const float4* sp = df.prev_pose + 4u * ((size_t)pr.z + local);
                    const float4 v0 = sp[0], v1 = sp[1], v2 = sp[2], gn = sp[3];
                    const float u = (float)(tr.y & 65535u) / 65535.0f, v = (float)(tr.y >> 16) / 65535.0f;
                    const float w = 1.0f - u - v;
                    const f3 pp = mk3((w * v0.x + u * v1.x) + v * v2.x, (w * v0.y + u * v1.y) + v * v2.y, (w * v0.z + u * v1.z) + v * v2.z);
                    const float4 a0 = rp[0], a1 = rp[1], a2 = rp[2], b1 = rp[4], b2 = rp[5];
                    P = xform_rows(a0, a1, a2, pp, 1.0f);
                    N = normalize(xform_rows(b0, b1, b2, mk3(gn.x, gn.y, gn.z), 0.0f));
                    if (tr.x & kDnFlipped) N = N * -1.0f;
                    state = 3u;
                }
            }
        }
        history = state != 0u;
    }
    if (history) {
        // where the primary hit P lay in the previous view: the ray pos' -> P cut with the image plane through p1' spanned by right', up'
        const f3 pos = mk3(tp.pos[0], tp.pos[1], tp.pos[2]), p1 = mk3(tp.p1[0], tp.p1[1], tp.p1[2]);
        const f3 right = mk3(tp.right[0], tp.right[1], tp.right[2]), up = mk3(tp.up[0], tp.up[1], tp.up[2]);
        const f3 d = P - pos, nrm = cross(right, up);
        const float num = dot(nrm, p1 - pos), den = dot(nrm, d);
        if (num * den > 0.0f) { // (else behind the previous camera)
            const f3 q = pos + (num / den) * d - p1;
            const float u = dot(q, right) / dot(right, right), v = dot(q, up) / dot(up, up);
            const float fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
            if (fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) { // (else no tap inside the frame; a NaN lands here too)
                const float ffx = __builtin_floorf(fx), ffy = __builtin_floorf(fy);
                const int i0 = (int)ffx, j0 = (int)ffy;
                const float tx = fx - ffx, ty = fy - ffy;
                const float inv_plane = 1.0f / (kDnPlane * g0.w);
                float sw = 0.0f, sh = 0.0f;
                f3 sx = mk3(0.0f);
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        const int qx = i0 + e, qy = j0 + b;
                        if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
                        const uint32_t k = (uint32_t)qx + (uint32_t)qy * cam.width;
                        const float4 xq = tp.prev[k];
                        if (!(xq.w > 0.0f)) continue;
                        if (MOTION && mp.prev_ids[k] != id) continue;
                        const float4 g0q = tp.prev[plane + k], g1q = tp.prev[2u * plane + k];
                        float wn = gl_max(0.0f, N.x * g0q.x + N.y * g0q.y + N.z * g0q.z);
                        for (int r = 0; r < kDnNormalSquarings; r++) wn = wn * wn;
                        const float dp = N.x * (g1q.x - P.x) + N.y * (g1q.y - P.y) + N.z * (g1q.z - P.z);
                        const float wp = gl_max(0.0f, 1.0f - gl_abs(dp) * inv_plane);
                        const float w = (e ? tx : 1.0f - tx) * (b ? ty : 1.0f - ty) * wn * wp;
                        sw += w;
                        sx = sx + w * mk3(xq.x, xq.y, xq.z);
                        sh += w * xq.w;
                    }
                if (sw >= kDnTemporalMinWeight) {
                    hh = gl_min(sh / sw, gl_max(tp.max_history - n, 0.0f));
                    if (hh > 0.0f) {
                        const f3 xh = mk3(sx.x / sw, sx.y / sw, sx.z / sw);
                        x = xh + (n / (hh + n)) * (c - xh);
                    }
                }
            }
        }
    }
    float h = hh + n;
    if (!(gl_abs(x.x) <= 3.0e38f && gl_abs(x.y) <= 3.0e38f && gl_abs(x.z) <= 3.0e38f)) h = 0.0f; // not finite: no history for the next image, and the passes leave it out
    tp.cur[i] = make_float4(x.x, x.y, x.z, h);
}

__global__ __launch_bounds__(kDnTile * kDnTile) void k_dn_temporal(const CameraParams cam, const DnTemporalParams tp)
{
    dn_temporal_pixel<false, false>(cam, tp, DnMotionParams{}, DnDeformParams{});
}

__global__ __launch_bounds__(kDnTile * kDnTile) void k_dn_temporal_motion(const CameraParams cam, const DnTemporalParams tp, const DnMotionParams mp)
{
    dn_temporal_pixel<true, false>(cam, tp, mp, DnDeformParams{});
}

__global__ __launch_bounds__(kDnTile * kDnTile) void k_dn_temporal_deform(const CameraParams cam, const DnTemporalParams tp, const DnMotionParams mp, const DnDeformParams df)
{
    dn_temporal_pixel<true, true>(cam, tp, mp, df);
}

void launch_dn_guide(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, float4* guide, uint32_t pixel_mask)
{
    if (p.capacity) hipLaunchKernelGGL(k_dn_guide, dim3((p.capacity + 255u) / 256u), dim3(256), 0, s, cam, sc, p, guide, pixel_mask);
}

void launch_dn_ids(hipStream_t s, const CameraParams& cam, const PathDev& p, uint32_t* ids, uint32_t pixel_mask)
{
    if (p.capacity) hipLaunchKernelGGL(k_dn_ids, dim3((p.capacity + 255u) / 256u), dim3(256), 0, s, cam, p, ids, pixel_mask);
}

void launch_dn_tris(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, uint2* tris, uint32_t pixel_mask)
{
    if (p.capacity) hipLaunchKernelGGL(k_dn_tris, dim3((p.capacity + 255u) / 256u), dim3(256), 0, s, cam, sc, p, tris, pixel_mask);
}

void launch_dn_pose(hipStream_t s, const rfw_rt_triangle* triangles, const uint4* copies, uint32_t n_copies, uint32_t total, float4* pose)
{
    if (n_copies && total) hipLaunchKernelGGL(k_dn_pose, dim3((4u * total + 255u) / 256u), dim3(256), 0, s, triangles, copies, n_copies, total, pose);
}

void launch_dn_motion(hipStream_t s, const rfw_mat4* matrices, const InstanceXform* xf, const InstanceNormal* nm, uint32_t n, const void* prev, uint32_t n_prev,
                      void* cur, void* records, const DnDeformMotion* deform)
{
    const DnDeformMotion d = deform ? *deform : DnDeformMotion{};
    if (n) hipLaunchKernelGGL(k_dn_motion, dim3((n + 63u) / 64u), dim3(64), 0, s, matrices, xf, nm, n, static_cast<const DnInstance*>(prev), n_prev,
                              static_cast<DnInstance*>(cur), static_cast<DnMotion*>(records), d.copies, d.n_copies, d.prev_refs, d.cur_refs);
}

template <bool TILED> static void launch_atrous_pass(hipStream_t s, const CameraParams& cam, const DnParams& dp, bool first, bool last)
{
    const uint32_t step = 1u << dp.step_shift;
    // TILED: the tiles of one sub-image ((width / step) x (height / step) pixels, rounded up), times step^2 sub-images, those fastest
    const dim3 grid = TILED ? dim3(ceil_div(ceil_div(cam.width, step), kDnTile) * step, ceil_div(ceil_div(cam.height, step), kDnTile) * step)
                            : dim3(ceil_div(cam.width, kDnTile), ceil_div(cam.height, kDnTile));
    const dim3 block(kDnTile * kDnTile);
    if (first && last) hipLaunchKernelGGL((k_atrous<true, true, TILED>), grid, block, 0, s, cam, dp);
    else if (first) hipLaunchKernelGGL((k_atrous<true, false, TILED>), grid, block, 0, s, cam, dp);
    else if (last) hipLaunchKernelGGL((k_atrous<false, true, TILED>), grid, block, 0, s, cam, dp);
    else hipLaunchKernelGGL((k_atrous<false, false, TILED>), grid, block, 0, s, cam, dp);
}

void launch_dn_temporal(hipStream_t s, const CameraParams& cam, const float4* acc, uint64_t slab_elems, const float4* guide, const float4* prev, float4* cur,
                        const float prev_view[12], uint32_t samples, uint32_t max_history, const DnMotionLaunch* motion, const DnDeformLaunch* deform)
{
    DnTemporalParams tp;
    tp.acc = acc;
    tp.slab_elems = slab_elems;
    tp.guide = guide;
    tp.prev = prev;
    tp.cur = cur;
    for (int k = 0; k < 3; k++) { tp.pos[k] = prev_view[k]; tp.p1[k] = prev_view[3 + k]; tp.right[k] = prev_view[6 + k]; tp.up[k] = prev_view[9 + k]; }
    tp.samples = samples;
    tp.max_history = (float)max_history;
    const dim3 grid(ceil_div(cam.width, kDnTile), ceil_div(cam.height, kDnTile)), block(kDnTile * kDnTile);
    if (motion == nullptr) {
        hipLaunchKernelGGL(k_dn_temporal, grid, block, 0, s, cam, tp);
        return;
    }
    DnMotionParams mp;
    mp.ids = motion->ids;
    mp.prev_ids = motion->prev_ids;
    mp.cur_ids = motion->cur_ids;
    mp.records = static_cast<const DnMotion*>(motion->records);
    mp.n_records = motion->n_records;
    if (deform == nullptr) {
        hipLaunchKernelGGL(k_dn_temporal_motion, grid, block, 0, s, cam, tp, mp);
        return;
    }
    DnDeformParams df;
    df.tris = deform->tris;
    df.refs = deform->refs;
    df.prev_refs = deform->prev_refs;
    df.prev_pose = deform->prev_pose;
    hipLaunchKernelGGL(k_dn_temporal_deform, grid, block, 0, s, cam, tp, mp, df);
}

void launch_atrous(hipStream_t s, const CameraParams& cam, const float4* acc, uint64_t slab_elems, const float4* guide, float4* const planes[2], float4* frame,
                   uint32_t samples, uint32_t passes, float sigma_colour, uint32_t form, const float4* x0)
{
    for (uint32_t i = 0; i < passes; i++) {
        DnParams dp;
        dp.acc = acc;
        dp.slab_elems = slab_elems;
        dp.guide = guide;
        dp.in = i ? planes[(i - 1u) & 1u] : x0;
        dp.out = i + 1u == passes ? frame : planes[i & 1u];
        dp.samples = samples;
        dp.step_shift = i;
        const float sigma = (float)((double)sigma_colour / (double)(1u << i) / std::sqrt((double)samples));
        dp.inv_sigma2 = (float)std::min(1.0 / ((double)sigma * (double)sigma), 3.0e38); // (finite: 0 x inf would poison equal colours)
        const bool tiled = form == 0u ? atrous_tiled_by_default(i) : form == 2u;
        const bool first = i == 0u && x0 == nullptr; // (x_0 handed in: every pass reads a plane)
        if (tiled) launch_atrous_pass<true>(s, cam, dp, first, i + 1u == passes);
        else launch_atrous_pass<false>(s, cam, dp, first, i + 1u == passes);
    }
}
