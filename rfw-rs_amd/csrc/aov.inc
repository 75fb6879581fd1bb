// aov.inc — the render modes other than the path tracer (rfw_hip_render's `mode`, rfw_backend::RenderMode; DESIGN.md "Render modes"),
// included by kernels.hip inside namespace rfwhip.
//
//   k_aov        after k_primary (any flavour): reads the camera ray's hit as k_shade does at bounce 0 and either adds the mode's value to
//                the accumulator slab (1 normal, 2 albedo, 3 G-buffer position + t, 4 view-space position) or (5, 6) files the ambient
//                occlusion rays into the shadow queue, round r in bucket r with ONE entry per slab slot, and writes the filter's guide
//   k_ao_filter  mode 6 where the frame is de-tiled on this device (world == 1): the edge-aware filter of ao = acc.x / n into the frame
//
// The AO rays are traced by launch_shadow, one launch per round: k_shadow's read-modify-write of the accumulator assumes one ray per slot
// per launch, which one round per launch keeps.  A ray that is not occluded adds 1 / ao_samples to the slot's rgb.

// the path-length slot of the xorshift seed the AO directions draw from: camera paths use 0 .. kMaxBounces - 1 (8), so this one is theirs alone
constexpr uint32_t kAoSeedSlot = 31u;
constexpr uint32_t kNoAoPixel = 0xffffffffu; // the pixel word of a queue entry that holds no AO ray (a miss, or a slab slot without a pixel)
constexpr int kAoFilterRadius = 3, kAoFilterTile = 16, kAoFilterSpan = kAoFilterTile + 2 * kAoFilterRadius;

struct AovParams {
    uint32_t mode;       // RFW_HIP_RENDER_NORMAL .. RFW_HIP_RENDER_FILTERED_SSAO
    uint32_t ao_samples; // 1 .. kAoMaxSamples
    float ao_radius;     // world units, > 0 (the host resolves "automatic")
    float4* guide;       // frame pixels: (faced gN, t) of the primary hit, (0, 0, 0, 0) where the camera ray missed
    float direction[3];  // the view's direction (mode 4; CameraParams carries right and up only)
};

// cosine-weighted direction about the unit normal n: (x, y, z) of DiffuseReflectionCosWeighted in the orthonormal basis of Duff et al.,
// "Building an Orthonormal Basis, Revisited" (JCGT 2017)
RFW_DI f3 cosine_about(const f3 n, const float r0, const float r1)
{
    const f3 l = DiffuseReflectionCosWeighted(r0, r1);
    const float sign = n.z >= 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sign + n.z), b = n.x * n.y * a;
    const f3 t = mk3(1.0f + sign * n.x * n.x * a, sign * b, -sign * n.x);
    const f3 bt = mk3(b, sign + n.y * n.y * a, -n.y);
    return normalize(t * l.x + bt * l.y + n * l.z);
}

// What the camera ray of a slab slot sees (S, O4, D4: k_primary's hit[0], ray_o[0], ray_d[0] of a slot whose ray HIT): k_shade at bounce 0,
// step for step (kernels.hip) — the same normal, tangent frame and material colour.  Shared by k_aov and the denoiser's guide (denoise.inc).
struct PrimarySurface {
    f3 P, gN, N, albedo; // O + t D, the faced geometric normal, the faced (normal-mapped) shading normal, material colour x diffuse map
    float t;
    bool light; // an emitter as k_shade sees it: a colour component above 1 and no emissive map
};
RFW_DI PrimarySurface primary_surface(const CameraParams& cam, const SceneDev& sc, const uint4 S, const float4 O4, const float4 D4)
{
    PrimarySurface ps;
    const f3 O = mk3(O4.x, O4.y, O4.z), D = mk3(D4.x, D4.y, D4.z);
    const int32_t INST_ID = (int32_t)S.x;
    const uint32_t TRI_ID = S.y;
    const float t_hit = bitsf(S.z);
    f3 P, gN;
    const float4* tp = reinterpret_cast<const float4*>(sc.triangles + TRI_ID);
    const float4 q3 = tp[3], q4 = tp[4], q5 = tp[5], q6 = tp[6], T0 = tp[7], T1 = tp[8], T2 = tp[9];
    const uint4 q10 = *reinterpret_cast<const uint4*>(tp + 10);
    ShadingData sd = extractParameters(sc.materials + (int32_t)q10.y);
    const float u = (float)(S.w & 65535u) * (1.0f / 65535.0f);
    const float v = (float)(S.w >> 16) * (1.0f / 65535.0f);
    const float w = 1.0f - u - v;
    gN = mk3(q3.x, q3.y, q3.z);
    f3 N = w * mk3(q4.x, q4.y, q4.z) + u * mk3(q5.x, q5.y, q5.z) + v * mk3(q6.x, q6.y, q6.z);
    f3 T = w * mk3(T0.x, T0.y, T0.z) + u * mk3(T1.x, T1.y, T1.z) + v * mk3(T2.x, T2.y, T2.z);
    const float Tw = w * T0.w + u * T1.w + v * T2.w;
    const float4* np = reinterpret_cast<const float4*>(sc.instance_normals + INST_ID);
    const float4 n0 = np[0], n1 = np[1], n2 = np[2];
    gN = normalize(xform_rows(n0, n1, n2, gN, 0.0f));
    N = normalize(xform_rows(n0, n1, n2, N, 0.0f));
    T = normalize(xform_rows(n0, n1, n2, T, 0.0f));
    const f3 B = cross(N, T) * Tw;
    P = O + t_hit * D;
    const bool light = (sd.color.x > 1.0f || sd.color.y > 1.0f || sd.color.z > 1.0f) && !(sd.flags & RFW_MAT_HAS_EMISSIVE_MAP);
    if ((sd.flags & 63u) != 0u) {
        const float lambda = __builtin_sqrtf(bitsf(q10.z)) + rfw_log2f(cam.spread_angle * (1.0f / gl_abs(dot(D, N))));
        const float4 q0 = tp[0], q1 = tp[1], q2 = tp[2];
        const float tu = w * q0.w + u * q1.w + v * q2.w;
        const float tv = w * q3.w + u * q4.w + v * q5.w;
        if (!light && (sd.flags & RFW_MAT_HAS_DIFFUSE_MAP) && sd.diffuse_map >= 0 && (uint32_t)sd.diffuse_map < sc.n_textures) {
            const f4 c = fetchTexelTrilinear(sc.tex_data, sc.tex_desc[sd.diffuse_map], lambda, tu, tv);
            sd.color = sd.color * mk3(c.x, c.y, c.z);
        }
        if (!light && (sd.flags & RFW_MAT_HAS_NORMAL_MAP) && sd.normal_map >= 0 && (uint32_t)sd.normal_map < sc.n_textures) {
            const f4 c = texture_sample(sc.tex_data, sc.tex_desc[sd.normal_map], tu, tv, (float)f2i(lambda));
            const f3 m = (mk3(c.x, c.y, c.z) - mk3(0.5f)) * 2.0f;
            N = normalize((T * m.x + B * m.y) + N * m.z);
        }
    }
    if (dot(D, gN) >= 0.0f) { // back facing
        N = N * -1.0f;
        gN = gN * -1.0f;
    }
    ps.P = P; ps.gN = gN; ps.N = N; ps.albedo = sd.color;
    ps.t = t_hit;
    ps.light = light;
    return ps;
}

__global__ __launch_bounds__(256) void k_aov(const CameraParams cam, const SceneDev sc, const PathDev p, const AovParams ap)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    const bool ao = ap.mode >= RFW_HIP_RENDER_SSAO;
    if (ao && idx == 0u)
        for (uint32_t r = 0; r < ap.ao_samples; r++) sc.counters->shadow[r][r] = p.capacity; // round r: bucket r of "bounce" r, every slot
    if (idx >= p.capacity) return;
    const uint4 S = p.hit[0][idx];
    const float4 O4 = p.ray_o[0][idx], D4 = p.ray_d[0][idx];
    const uint32_t path_id = fbits(O4.w);
    const bool pixel = S.x != kNoPath, hit = pixel && (int32_t)S.x >= 0;
    float4 value = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    f3 P = mk3(0.0f), gN = mk3(0.0f);
    float t_hit = 0.0f;
    if (hit) {
        const PrimarySurface ps = primary_surface(cam, sc, S, O4, D4);
        const f3 N = ps.N;
        P = ps.P;
        gN = ps.gN;
        t_hit = ps.t;
        if (ap.mode == RFW_HIP_RENDER_NORMAL) value = make_float4(N.x, N.y, N.z, 0.0f);
        else if (ap.mode == RFW_HIP_RENDER_ALBEDO) value = make_float4(ps.albedo.x, ps.albedo.y, ps.albedo.z, 0.0f);
        else if (ap.mode == RFW_HIP_RENDER_GBUFFER) value = make_float4(P.x, P.y, P.z, t_hit);
        else if (ap.mode == RFW_HIP_RENDER_SCREEN_SPACE) {
            const f3 pos = mk3(cam.pos[0], cam.pos[1], cam.pos[2]), rel = P - pos;
            const f3 rh = normalize(mk3(cam.right[0], cam.right[1], cam.right[2])), uh = normalize(mk3(cam.up[0], cam.up[1], cam.up[2]));
            const f3 dh = normalize(mk3(ap.direction[0], ap.direction[1], ap.direction[2]));
            value = make_float4(dot(rel, rh), dot(rel, uh), dot(rel, dh), 1.0f);
        }
    }
    if (!ao) {
        if (pixel) {
            float4 a = p.acc[idx];
            a.x += value.x; a.y += value.y; a.z += value.z; a.w += value.w;
            p.acc[idx] = a;
        }
        return;
    }
    if (pixel) ap.guide[path_id] = hit ? make_float4(gN.x, gN.y, gN.z, t_hit) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t seed = wang_hash(path_id * 16789u + cam.sample_count * 1791u + kAoSeedSlot * 720898027u);
    const float e = 1.0f / (float)(int)ap.ao_samples;
    for (uint32_t r = 0; r < ap.ao_samples; r++) {
        const size_t j = (size_t)r * p.capacity + idx;
        if (hit) {
            const float r0 = randf(seed), r1 = randf(seed);
            const f3 R = cosine_about(gN, r0, r1);
            const f3 o = safe_origin(P, R, gN);
            p.sh_o[j] = make_float4(o.x, o.y, o.z, bitsf(path_id));
            p.sh_d[j] = make_float4(R.x, R.y, R.z, ap.ao_radius + 0.0001f); // (k_shadow traces to d.w - 1e-4)
            p.sh_e[j] = make_float4(e, e, e, bitsf(idx));
        } else { // an entry that adds nothing: t_max < t_min
            p.sh_o[j] = make_float4(0.0f, 0.0f, 0.0f, bitsf(kNoAoPixel));
            p.sh_d[j] = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
            p.sh_e[j] = make_float4(0.0f, 0.0f, 0.0f, bitsf(idx));
        }
    }
}

// out(p) = sum_q w(p, q) ao(q) / sum_q w(p, q) over the (2R + 1)^2 window clipped to the frame, R = 3,
// w(p, q) = max(0, dot(Np, Nq))^8 * max(0, 1 - |tp - tq| / (0.05 tp)), w = 0 where q missed; 0 where p missed (DESIGN.md "Render modes").
// One workgroup per 16 x 16 pixels; the 22 x 22 window of ao and guide is staged in LDS once.
__global__ __launch_bounds__(kAoFilterTile * kAoFilterTile) void k_ao_filter(const CameraParams cam, const float4* __restrict__ acc, const uint64_t slab_elems,
                                                                              const float4* __restrict__ guide, float4* __restrict__ frame, const uint32_t samples)
{
    __shared__ float s_ao[kAoFilterSpan * kAoFilterSpan];
    __shared__ float4 s_g[kAoFilterSpan * kAoFilterSpan];
    const int x0 = (int)(blockIdx.x * kAoFilterTile) - kAoFilterRadius, y0 = (int)(blockIdx.y * kAoFilterTile) - kAoFilterRadius;
    const float n = (float)(int)samples;
    for (int k = (int)threadIdx.x; k < kAoFilterSpan * kAoFilterSpan; k += kAoFilterTile * kAoFilterTile) {
        const int x = x0 + k % kAoFilterSpan, y = y0 + k / kAoFilterSpan;
        float a = 0.0f;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // outside the frame: weight 0, as a miss
        if (x >= 0 && y >= 0 && x < (int)cam.width && y < (int)cam.height) {
            uint32_t owner;
            const uint32_t slot = pixel_to_slab(cam, (uint32_t)x, (uint32_t)y, owner);
            a = acc[(uint64_t)owner * slab_elems + slot].x * 1.0f / n;
            g = guide[(uint32_t)x + (uint32_t)y * cam.width];
        }
        s_ao[k] = a;
        s_g[k] = g;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x % kAoFilterTile), ly = (int)(threadIdx.x / kAoFilterTile);
    const int px = x0 + kAoFilterRadius + lx, py = y0 + kAoFilterRadius + ly;
    if (px >= (int)cam.width || py >= (int)cam.height) return;
    const float4 gp = s_g[(ly + kAoFilterRadius) * kAoFilterSpan + lx + kAoFilterRadius];
    float out = 0.0f;
    if (gp.w > 0.0f) {
        float sw = 0.0f, swa = 0.0f;
        for (int dy = 0; dy <= 2 * kAoFilterRadius; dy++)
            for (int dx = 0; dx <= 2 * kAoFilterRadius; dx++) {
                const int k = (ly + dy) * kAoFilterSpan + lx + dx;
                const float4 gq = s_g[k];
                if (!(gq.w > 0.0f)) continue;
                float c = gl_max(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z);
                c = c * c; c = c * c; c = c * c;
                const float wt = c * gl_max(0.0f, 1.0f - gl_abs(gp.w - gq.w) / (0.05f * gp.w));
                sw += wt;
                swa += wt * s_ao[k];
            }
        out = sw > 0.0f ? swa / sw : 0.0f;
    }
    frame[(uint32_t)px + (uint32_t)py * cam.width] = make_float4(out, out, out, 0.0f);
}

void launch_aov(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, uint32_t mode, uint32_t ao_samples, float ao_radius, float4* guide,
                const float direction[3])
{
    AovParams ap;
    ap.mode = mode;
    ap.ao_samples = ao_samples;
    ap.ao_radius = ao_radius;
    ap.guide = guide;
    for (int c = 0; c < 3; c++) ap.direction[c] = direction[c];
    if (p.capacity) hipLaunchKernelGGL(k_aov, dim3((p.capacity + 255u) / 256u), dim3(256), 0, s, cam, sc, p, ap);
}
void launch_ao_filter(hipStream_t s, const CameraParams& cam, const float4* acc, uint64_t slab_elems, const float4* guide, float4* frame, uint32_t samples)
{
    const dim3 grid((cam.width + kAoFilterTile - 1) / kAoFilterTile, (cam.height + kAoFilterTile - 1) / kAoFilterTile);
    hipLaunchKernelGGL(k_ao_filter, grid, dim3(kAoFilterTile * kAoFilterTile), 0, s, cam, acc, slab_elems, guide, frame, samples);
}
