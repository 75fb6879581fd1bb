// traverse_leaf.inc — one mesh leaf (included by both loop shapes): Moeller-Trumbore over the leaf's 48-B triangle packets.
// Hook: RFW_TRAV_OCCLUDED (any hit: a triangle blocks the ray).
            // ---- BLAS leaf: Moeller-Trumbore over the packets (intersection.glsl:1-38 / 40-70)
            const uint32_t first = cur & kLeafFirstMask, count = ((cur >> 27) & 15u) + 1u;
            const float4* tp = reinterpret_cast<const float4*>(sc.tri_packets + tri_base + first);
            for (uint32_t k = 0; k < count; k++) {
                const float4 p0 = tp[3 * k], p1 = tp[3 * k + 1], p2 = tp[3 * k + 2];
                if (COUNT) {
                    tc.tris++;
                    if (__builtin_amdgcn_mbcnt_hi((uint32_t)(__ballot(1) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)__ballot(1), 0u)) == 0u) tc.wave_tris++;
                }
                const f3 v0 = mk3(p0.x, p0.y, p0.z), edge1 = mk3(p1.x, p1.y, p1.z), edge2 = mk3(p2.x, p2.y, p2.z);
                // The same operations in the same order as intersection.glsl:1-38 / 40-70, WITHOUT its early outs: in a wavefront of ~11 lanes at
                // leaves some lane passes every test but the last almost every time, so the early outs skip nothing — and each is an exec-mask
                // update, a branch, and (the compiler sinks the v0 load behind the first) a dependent load.  A rejected candidate's later
                // values are never used: where a ~ 0 they may be inf / NaN, and every comparison with a NaN is false as in the original.
                const f3 h = cross(d, edge2);
                const float a = dot(edge1, h);
                const float f = 1.0f / a;
                const f3 s = o - v0;
                const float u = f * dot(s, h);
                const f3 q = cross(s, edge1);
                const float v = f * dot(d, q);
                const float tt = f * dot(edge2, q);
                const bool ok = !((a > -0.0001f) & (a < 0.0001f)) & !((u < 0.0f) | (u > 1.0f)) & !((v < 0.0f) | ((u + v) > 1.0f));
                if (ANY_HIT) {
                    if (ok & (tt > t_min) & (tt < t)) { RFW_TRAV_OCCLUDED }
                } else {
                    const int32_t prim = (int32_t)fbits(p0.w);
                    const int32_t inst_ = SS ? (int32_t)fbits(p2.w) : cur_inst; // (SS: the packet names its mesh's one instance)
                    const bool lower = (inst_ < hit_inst) | ((inst_ == hit_inst) & (prim < hit_tri));
                    const bool take = ok & (tt > t_min) & ((tt < t) | ((tt == t) & (hit_inst >= 0) & lower));
                    t = take ? tt : t;
                    hu = take ? u * p1.w : hu;
                    hv = take ? v * p1.w : hv;
                    hit_inst = take ? inst_ : hit_inst;
                    hit_tri = take ? prim : hit_tri;
                }
            }
