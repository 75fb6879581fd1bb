// shade_kernel.inc — the body of the shade kernel (shade.comp:70-266), included once per twin by kernels.hip: k_shade with MAPS = false,
// k_shade_maps with MAPS = true (option "material_maps").  In scope: BATCH, kShadeBlock, MAPS, and the kernel's arguments cam, sc, p, bounce.
    static_assert(kShadeBlock >= 128 && 8 * (kShadeBlock / 64) <= 64, "k_shade: the extension-ray filing needs a second wavefront and at most 64 (octant, wavefront) counts");
    const uint32_t idx = blockIdx.x * kShadeBlock + threadIdx.x;
    const uint32_t count = bounce == 0 ? p.capacity : sc.counters->ext[bounce - 1];
    if (blockIdx.x * kShadeBlock >= count) return;
    const uint32_t half = bounce & 1u, next_half = half ^ 1u;
    const uint32_t path_length = bounce;

    bool live = idx < count;

    bool push_ext = false, push_shadow = false;
    int light_bucket = 0;
    f3 ext_o = mk3(0.0f), ext_d = mk3(0.0f), ext_thr = mk3(0.0f);
    float ext_pdf = 0.0f;
    uint32_t ext_normal = 0;
    f3 sh_o = mk3(0.0f), sh_d = mk3(0.0f), sh_e = mk3(0.0f);
    float sh_dist = 0.0f;
    uint32_t PATH_ID = 0, PATH_WORD = 0, sh_slot = 0;

    uint4 S = make_uint4(kNoPath, 0u, 0u, 0u);
    if (live) {
        S = p.hit[half][idx];
        live = S.x != kNoPath; // bounce 0: a slab slot of a ragged edge tile that holds no pixel (marked by k_primary)
    }
    if (live) {
        const float4 O4 = p.ray_o[half][idx], D4 = p.ray_d[half][idx];
        const f3 O = mk3(O4.x, O4.y, O4.z), D = mk3(D4.x, D4.y, D4.z);
        f3 throughput = mk3(1.0f);
        float bsdfPdf = 1.0f;
        if (path_length != 0) {
            const float4 T4 = p.thr[half][idx];
            throughput = mk3(T4.x, T4.y, T4.z);
            bsdfPdf = T4.w;
        }
        const uint32_t path_word = fbits(O4.w); // batch: frame index in the top byte
        PATH_ID = BATCH ? (path_word & 0xffffffu) : path_word;
        PATH_WORD = path_word;
        // bounce 0: path idx of the (tall) virtual frame IS its accumulator slot; later bounces recompute it from the pixel
        uint32_t owner, slot = idx;
        if (bounce != 0) {
            const uint32_t py_ = div_magic(PATH_ID, cam.width, cam.width_magic);
            slot = pixel_to_slab(cam, PATH_ID - py_ * cam.width, py_, owner) + (BATCH ? (path_word >> 24) * cam.frame_capacity : 0u);
        }
        const int32_t INST_ID = (int32_t)S.x;
        const uint32_t TRI_ID = S.y;
        const float T_VAL = bitsf(S.z);

        if (INST_ID < 0) { // shade.comp:90-96: lat-long skybox lookup at LOD = path length (constant sky colour when none is set)
            f3 sky = mk3(cam.sky[0], cam.sky[1], cam.sky[2]);
            if (sc.skybox.mips) {
                const float su = 0.5f * (1.0f + rfw_atan2f(D.x, -D.z) * (1.0f / 3.14159265359f));
                const float sv = 1.0f - rfw_acosf(D.y) * (1.0f / 3.14159265359f);
                const f4 c = texture_sample(sc.tex_data, sc.skybox, su, sv, (float)(int)path_length);
                sky = mk3(c.x, c.y, c.z);
            }
            f3 contribution = throughput * sky * (1.0f / bsdfPdf);
            CLAMPINTENSITY(contribution, cam.clamp_value);
            float4 a = p.acc[slot];
            a.x += contribution.x; a.y += contribution.y; a.z += contribution.z; a.w += 0.0f;
            p.acc[slot] = a;
        } else {
            // 176-B RTTriangle as 11 dwordx4 loads (only here, once per shaded hit)
            const float4* tp = reinterpret_cast<const float4*>(sc.triangles + TRI_ID);
            const float4 q3 = tp[3], q4 = tp[4], q5 = tp[5], q6 = tp[6], T0 = tp[7], T1 = tp[8], T2 = tp[9];
            const uint4 q10 = *reinterpret_cast<const uint4*>(tp + 10);
            const int32_t mat_id = (int32_t)q10.y;
            const float tri_area = bitsf(q10.w);
            ShadingData sd = extractParameters<MAPS>(sc.materials + mat_id);

            // shade.comp:102: pathId / (w * h) + sample count, and a path id is a pixel index here; a frame of a batch carries its own sample index
            const uint32_t sampleId = BATCH ? cam.batch_sample[path_word >> 24] : cam.sample_count;
            uint32_t seed = wang_hash(PATH_ID * 16789u + sampleId * 1791u + path_length * 720898027u);

            const float u = (float)(S.w & 65535u) * (1.0f / 65535.0f);
            const float v = (float)(S.w >> 16) * (1.0f / 65535.0f);
            const float w = 1.0f - u - v;

            f3 gN = mk3(q3.x, q3.y, q3.z);
            f3 N = w * mk3(q4.x, q4.y, q4.z) + u * mk3(q5.x, q5.y, q5.z) + v * mk3(q6.x, q6.y, q6.z);
            f3 T = w * mk3(T0.x, T0.y, T0.z) + u * mk3(T1.x, T1.y, T1.z) + v * mk3(T2.x, T2.y, T2.z);
            const float Tw = w * T0.w + u * T1.w + v * T2.w;

            const float4* np = reinterpret_cast<const float4*>(sc.instance_normals + INST_ID);
            const float4 n0 = np[0], n1 = np[1], n2 = np[2];
            gN = normalize(xform_rows(n0, n1, n2, gN, 0.0f));
            N = normalize(xform_rows(n0, n1, n2, N, 0.0f));
            T = normalize(xform_rows(n0, n1, n2, T, 0.0f));
            const f3 B = cross(N, T) * Tw;
            const f3 P = O + T_VAL * D;

            const bool any_map = (sd.flags & 63u) != 0u;
            // shade.comp:128-160 hit a light (a material with an emissive map is shaded as a surface instead)
            if ((sd.color.x > 1.0f || sd.color.y > 1.0f || sd.color.z > 1.0f) && !(sd.flags & RFW_MAT_HAS_EMISSIVE_MAP)) {
                f3 contribution = mk3(0.0f);
                const float DdotNL = -dot(D, N);
                bool add = true;
                if (DdotNL > 0.0f) {
                    if (path_length == 0) {
                        contribution = throughput * sd.color * (1.0f / bsdfPdf);
                    } else {
                        const float lightPdf = CalculateLightPDF(D, T_VAL, tri_area, N);
                        const int lc = (int)(cam.area_light_count + cam.point_light_count + cam.spot_light_count + cam.directional_light_count);
                        const float pickProb = 1.0f / (float)lc;
                        if ((bsdfPdf + lightPdf * pickProb) <= 0.0f) add = false;
                        else contribution = throughput * sd.color * (1.0f / (bsdfPdf + lightPdf * pickProb));
                    }
                    CLAMPINTENSITY(contribution, cam.clamp_value);
                }
                if (add) {
                    float4 a = p.acc[slot];
                    a.x += contribution.x; a.y += contribution.y; a.z += contribution.z; a.w += 0.0f;
                    p.acc[slot] = a;
                }
            } else {
                bool dim = false; // MAPS: no component of the material's own colour exceeds 1 (else an emissive map is not live)
                if constexpr (MAPS) dim = !(sd.color.x > 1.0f || sd.color.y > 1.0f || sd.color.z > 1.0f);
                if (any_map) { // shade.comp:162-175
                    const float lambda = __builtin_sqrtf(bitsf(q10.z)) + rfw_log2f(cam.spread_angle * (1.0f / gl_abs(dot(D, N))));
                    const float4 q0 = tp[0], q1 = tp[1], q2 = tp[2];
                    const float tu = w * q0.w + u * q1.w + v * q2.w;   // u0, u1, u2 ride in the .w of the vertex slots
                    const float tv = w * q3.w + u * q4.w + v * q5.w;   // v0, v1, v2 in the .w of normal / n0 / n1
                    if ((sd.flags & RFW_MAT_HAS_DIFFUSE_MAP) && sd.diffuse_map >= 0 && (uint32_t)sd.diffuse_map < sc.n_textures) {
                        const f4 c = fetchTexelTrilinear(sc.tex_data, sc.tex_desc[sd.diffuse_map], lambda, tu, tv);
                        sd.color = sd.color * mk3(c.x, c.y, c.z);
                    }
                    if ((sd.flags & RFW_MAT_HAS_NORMAL_MAP) && sd.normal_map >= 0 && (uint32_t)sd.normal_map < sc.n_textures) {
                        const f4 c = texture_sample(sc.tex_data, sc.tex_desc[sd.normal_map], tu, tv, (float)f2i(lambda));
                        const f3 m = (mk3(c.x, c.y, c.z) - mk3(0.5f)) * 2.0f;
                        N = normalize((T * m.x + B * m.y) + N * m.z); // mat3(T, B, N) * m
                    }
                    if constexpr (MAPS) {
                        f3 Le;
                        // an emissive map radiates from the front side, at every bounce with weight 1 (next-event estimation never samples
                        // these triangles): the light branch's expression at path length 0; the hit is then shaded as a surface
                        if (apply_parameter_maps(sd, dim, sc.tex_data, sc.tex_desc, sc.n_textures, lambda, tu, tv, Le) && dot(D, gN) < 0.0f) {
                            f3 contribution = throughput * Le * (1.0f / bsdfPdf);
                            CLAMPINTENSITY(contribution, cam.clamp_value);
                            float4 a = p.acc[slot];
                            a.x += contribution.x; a.y += contribution.y; a.z += contribution.z; a.w += 0.0f;
                            p.acc[slot] = a;
                        }
                    }
                }
                prepare_tint(sd);
                const bool backFacing = dot(D, gN) >= 0.0f;
                if (backFacing) {
                    N = N * -1.0f;
                    gN = gN * -1.0f;
                }
                throughput = throughput * (1.0f / bsdfPdf);
                float newBsdfPdf = 0.0f;
                f3 R = mk3(0.0f);
                float r1, r2;
                const bool blue = sc.blue_noise != nullptr && sampleId < 256u; // shade.comp:189-195; the xorshift seed is not advanced on this branch
                const int by = (int)div_magic(PATH_ID, cam.width, cam.width_magic), bx = (int)(PATH_ID - (uint32_t)by * cam.width);
                if (blue) {
                    r1 = blueNoiseSampler(sc.blue_noise, sampleId, bx, by, (int)(4u + 4u * path_length));
                    r2 = blueNoiseSampler(sc.blue_noise, sampleId, bx, by, (int)(5u + 4u * path_length));
                } else {
                    r1 = randf(seed);
                    r2 = randf(seed);
                }
                const float F_gN = Fr_of(sd, dot(gN, D * -1.0f)); // the Fresnel term both pdfs of this hit use (sampled direction, light direction: same normal, same wo)
                const f3 bsdf = SampleBSDF(sd, N, gN, T, B, D * -1.0f, T_VAL, backFacing, r1, r2, R, newBsdfPdf, F_gN);
                throughput = throughput * bsdf * gl_abs(dot(N, R));
                throughput = gl_max(throughput, mk3(0.0f));
                if (!(newBsdfPdf <= 1e-4f || gl_isnan(newBsdfPdf))) {
                    const int lc = (int)(cam.area_light_count + cam.point_light_count + cam.spot_light_count + cam.directional_light_count);
                    if (!(cam.flags & kFlagNoNee) && lc > 0) {
                        float r3; // r4 (dimension 7 + 4 * path length, or the next xorshift draw) is drawn by the reference and never used
                        if (blue) r3 = blueNoiseSampler(sc.blue_noise, sampleId, bx, by, (int)(6u + 4u * path_length)); // shade.comp:216-221
                        else r3 = randf(seed);
                        LightView lv;
                        lv.area = sc.area_lights; lv.point = sc.point_lights; lv.spot = sc.spot_lights; lv.directional = sc.directional_lights;
                        lv.n_area = (int)cam.area_light_count; lv.n_point = (int)cam.point_light_count;
                        lv.n_spot = (int)cam.spot_light_count; lv.n_directional = (int)cam.directional_light_count;
                        f3 lightColor = mk3(0.0f);
                        float pickProb = 0.0f, lightPdf = 0.0f;
                        int picked = 0;
                        f3 L = RandomPointOnLight(lv, r3, P, N, pickProb, lightPdf, lightColor, picked) - P;
                        const float dist = length(L);
                        L = L * (1.0f / dist);
                        const float NdotL = dot(L, N);
                        if (NdotL > 0.0f && lightPdf > 0.0f) {
                            float shadowPdf = 0.0f;
                            const f3 sampledBSDF = EvaluateBSDF(sd, gN, D * -1.0f, L, shadowPdf, F_gN);
                            if (shadowPdf > 0.0f) {
                                f3 contribution = throughput * sampledBSDF * lightColor * (NdotL / (lightPdf * pickProb));
                                if (!(gl_isnan(contribution.x) || gl_isnan(contribution.y) || gl_isnan(contribution.z))) {
                                    CLAMPINTENSITY(contribution, cam.clamp_value);
                                    sh_o = safe_origin(P, L, gN);
                                    sh_d = L;
                                    sh_dist = dist - 1e-4f;
                                    sh_e = contribution;
                                    sh_slot = slot;
                                    push_shadow = true;
                                    // directional lights share the LAST bucket (their rays are traced far to near, k_shadow), the positional lights
                                    // are dealt over the other seven: the bucket tells the kind of light however many lights there are
                                    light_bucket = picked >= lc - (int)cam.directional_light_count ? kShadowBuckets - 1 : (int)((uint32_t)picked % (uint32_t)(kShadowBuckets - 1));
                                }
                            }
                        }
                    }
                    // the reference pushes the extension unconditionally (shade.comp:260-265) and its host loop simply stops
                    // after the last bounce; nothing reads that last queue, so it is not written here
                    if (bounce + 1 < cam.max_path_length) {
                        ext_o = safe_origin(P, R, gN);
                        ext_d = R;
                        ext_normal = PackNormal(N);
                        ext_thr = throughput;
                        ext_pdf = newBsdfPdf;
                        push_ext = true;
                    }
                }
            }
        }
    }

    // ---- queue compaction: ballot + mbcnt prefix inside each wavefront, wave totals combined through LDS, ONE atomic per
    // workgroup and queue (the reference issues one global atomic per thread, shade.comp:250,261; one per wavefront still
    // serialised 32 k returning atomics on a single address)
    constexpr int kQ = kShadowBuckets + 1; // queues: one shadow region per light bucket + the extension queue
    __shared__ uint32_t s_cnt[kQ][kShadeBlock / 64];
    __shared__ uint32_t s_base[kQ];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t my_rank = 0;
    for (int q = 0; q < kShadowBuckets; q++) {
        const bool mine = push_shadow && light_bucket == q;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) s_cnt[q][wave] = (uint32_t)__popcll(m);
        if (mine) my_rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    }
    // The extension rays of a workgroup go into its range of the queue OCTANT BY OCTANT of their direction (round 4): the trace kernels read
    // the copy of the tree made for a ray's octant, so a wavefront whose 64 consecutive entries share one or two octants touches one or two
    // copies of every node instead of up to eight (measured: k_extend 1.63 -> 1.54 ms per frame alone; +0.4 ... 2.5 % frame rate path traced).  The queue order
    // never shows in the image.
    __shared__ uint32_t s_ext[8][kShadeBlock / 64]; // [octant][wavefront]: count, then exclusive offset inside the workgroup's range
    const bool any_ext = bounce + 1 < cam.max_path_length; // (uniform)
    const uint32_t ext_oct = (fbits(ext_d.x) >> 31) | ((fbits(ext_d.y) >> 31) << 1) | ((fbits(ext_d.z) >> 31) << 2);
    uint32_t r_ex = 0;
    if (any_ext) {
        uint32_t total_wave = 0;
        for (uint32_t o8 = 0; o8 < 8u; o8++) {
            const bool mine = push_ext && ext_oct == o8;
            const unsigned long long m = __ballot(mine);
            if (lane == 0) s_ext[o8][wave] = (uint32_t)__popcll(m);
            if (mine) r_ex = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            total_wave += (uint32_t)__popcll(m);
        }
        if (lane == 0) s_cnt[kShadowBuckets][wave] = total_wave;
    } else if (lane == 0) s_cnt[kShadowBuckets][wave] = 0u;
    __syncthreads();
    if (threadIdx.x < kQ) {
        uint32_t tot = 0;
        for (int k = 0; k < kShadeBlock / 64; k++) tot += s_cnt[threadIdx.x][k];
        uint32_t base = 0;
        if (tot) base = atomicAdd(threadIdx.x < kShadowBuckets ? &sc.counters->shadow[bounce][threadIdx.x] : &sc.counters->ext[bounce], tot);
        s_base[threadIdx.x] = base;
    }
    uint32_t ext_before = 0;
    constexpr uint32_t kExtCounts = 8u * (kShadeBlock / 64);
    if (any_ext && threadIdx.x >= 64u && threadIdx.x < 64u + kExtCounts) { // the second wavefront: (octant, wavefront) t's offset = everything filed before it, octant-major
        const uint32_t t8 = threadIdx.x - 64u;
        const uint32_t* flat = &s_ext[0][0];
        for (uint32_t k = 0; k < t8; k++) ext_before += flat[k];
    }
    __syncthreads();
    if (any_ext && threadIdx.x >= 64u && threadIdx.x < 64u + kExtCounts) (&s_ext[0][0])[threadIdx.x - 64u] = ext_before;
    __syncthreads();
    if (push_shadow) {
        uint32_t off = s_base[light_bucket];
        for (uint32_t k = 0; k < wave; k++) off += s_cnt[light_bucket][k];
        const size_t j = (size_t)light_bucket * p.capacity + off + my_rank;
        p.sh_o[j] = make_float4(sh_o.x, sh_o.y, sh_o.z, bitsf(PATH_WORD));
        p.sh_d[j] = make_float4(sh_d.x, sh_d.y, sh_d.z, sh_dist);
        p.sh_e[j] = make_float4(sh_e.x, sh_e.y, sh_e.z, bitsf(sh_slot));
    }
    if (push_ext) {
        const uint32_t j = s_base[kShadowBuckets] + s_ext[ext_oct][wave] + r_ex;
        p.ray_o[next_half][j] = make_float4(ext_o.x, ext_o.y, ext_o.z, bitsf(PATH_WORD));
        p.ray_d[next_half][j] = make_float4(ext_d.x, ext_d.y, ext_d.z, bitsf(ext_normal));
        p.thr[next_half][j] = make_float4(ext_thr.x, ext_thr.y, ext_thr.z, ext_pdf);
    }
