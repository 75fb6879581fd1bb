// traverse_node.inc — one visit of an interior node (included by both loop shapes): the 4-wide slab test on the quantised child boxes of the
// copy made for the ray's octant, the hit children pushed in stored order.  Leaves `cur` = kInvalidRef ("take the next stack entry").
            // ---- interior node: 4-wide slab test on the quantised child boxes (64 B = 4 dwordx4 per lane)
            const uint4* np = reinterpret_cast<const uint4*>(nodes + cur);
            const uint4 w0 = np[0], w1 = np[1], w2 = np[2], ch = np[3];
            if (COUNT) {
                tc.nodes++;
                if (__builtin_amdgcn_mbcnt_hi((uint32_t)(__ballot(1) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)__ballot(1), 0u)) == 0u) {
                    tc.wave_nodes++;
                }
                {
                    const uint64_t first_ptr = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uintptr_t)np >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uintptr_t)np);
                    const bool all_same = __ballot((uintptr_t)np == first_ptr) == __ballot(1);
                    if (all_same && __builtin_amdgcn_mbcnt_hi((uint32_t)(__ballot(1) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)__ballot(1), 0u)) == 0u) tc.wave_uniform++;
                }
            }
            // plane = origin + q * scale  =>  t = q * (scale * inv) + (origin - o) * inv : one cvt + one fma per plane.  The node is the copy for
            // this ray's octant: qlo = the planes the ray enters through, qhi = the ones it leaves through, children front to back.
            const float Ax = bitsf(w0.w) * inv.x, Ay = bitsf(w2.z) * inv.y, Az = bitsf(w2.w) * inv.z;
            const float Bx = (bitsf(w0.x) - o.x) * inv.x, By = (bitsf(w0.y) - o.y) * inv.y, Bz = (bitsf(w0.z) - o.z) * inv.z;
            const v2f Ax2 = {Ax, Ax}, Ay2 = {Ay, Ay}, Az2 = {Az, Az}, Bx2 = {Bx, Bx}, By2 = {By, By}, Bz2 = {Bz, Bz};
            bool hit[4];
            // tf >= tn && tn <= t  <=>  min(tf, t) >= tn.  A NaN (0 * inf on an axis-parallel ray) is ignored by max3 / min3 and only drops that axis'
            // constraint; a direction of exact zeros makes tn NaN on every axis and fails the compare (the ray misses everything, as it must)
#define RFW_SLAB(i, CH)                                                                                                               \
    {                                                                                                                                 \
        const v2f qx = {(float)((w1.x >> (8 * i)) & 0xffu), (float)((w1.w >> (8 * i)) & 0xffu)};                                      \
        const v2f qy = {(float)((w1.y >> (8 * i)) & 0xffu), (float)((w2.x >> (8 * i)) & 0xffu)};                                      \
        const v2f qz = {(float)((w1.z >> (8 * i)) & 0xffu), (float)((w2.y >> (8 * i)) & 0xffu)};                                      \
        const v2f tx = __builtin_elementwise_fma(qx, Ax2, Bx2), ty = __builtin_elementwise_fma(qy, Ay2, By2),                         \
                  tz = __builtin_elementwise_fma(qz, Az2, Bz2);                                                                       \
        const float tn = __builtin_fmaxf(__builtin_fmaxf(tx.x, ty.x), tz.x);                                                          \
        const float tf = __builtin_fminf(__builtin_fminf(tx.y, ty.y), tz.y);                                                          \
        hit[i] = (__builtin_fminf(tf, t) >= __builtin_fmaxf(tn, 0.0f)) & (CH != kInvalidRef);                                         \
    }
            RFW_SLAB(0, ch.x)
            RFW_SLAB(1, ch.y)
            RFW_SLAB(2, ch.z)
            RFW_SLAB(3, ch.w)
#undef RFW_SLAB
            // The hit children go on the stack in reverse stored order (any hit from the far end: in stored order), without a branch: every child
            // is written to the slot above the hit ones so far, and the slot only advances past a hit — then the nearest comes back off the top.
            if (sp + 4 <= kStack) {
                uint32_t* slot = lds_stack + sp * kTraceBlock + lane_slot;
                constexpr bool kFwd = ANY_HIT && FAR_FIRST;
                const uint32_t c0 = kFwd ? ch.x : ch.w, c1 = kFwd ? ch.y : ch.z, c2 = kFwd ? ch.z : ch.y, c3 = kFwd ? ch.w : ch.x;
                const bool h0 = kFwd ? hit[0] : hit[3], h1 = kFwd ? hit[1] : hit[2], h2 = kFwd ? hit[2] : hit[1], h3 = kFwd ? hit[3] : hit[0];
                slot[0] = c0; slot += h0 ? kTraceBlock : 0;
                slot[0] = c1; slot += h1 ? kTraceBlock : 0;
                slot[0] = c2; slot += h2 ? kTraceBlock : 0;
                slot[0] = c3;
                sp += (h0 ? 1 : 0) + (h1 ? 1 : 0) + (h2 ? 1 : 0) + (h3 ? 1 : 0);
            } else {
                constexpr bool kFwd = ANY_HIT && FAR_FIRST;
                if (kFwd) { if (hit[0]) push(ch.x); if (hit[1]) push(ch.y); if (hit[2]) push(ch.z); if (hit[3]) push(ch.w); }
                else { if (hit[3]) push(ch.w); if (hit[2]) push(ch.z); if (hit[1]) push(ch.y); if (hit[0]) push(ch.x); }
            }
            if (COUNT && SS && cur >= sc.ss_root) gtop = sp; // a graft node: what lies on the stack now are graft nodes and meshes' roots (traverse.h, count_root)
            cur = kInvalidRef; // (falls through to the pop below)
