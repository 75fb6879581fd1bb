// traverse_nested.inc — the NESTED traversal loop of traverse.h (rounds 1-4): the plain closest-hit traversal keeps it, because both flat
// shapes cost that loop 15-20 % where it matters (scenes beyond the packets' range, latency-bound in HBM: EXPERIMENTS.md, round 5).
    for (;;) {
        if (!(cur & kLeafBit)) {
#include "traverse_node.inc"
        } else if (SS || blas_sp >= 0) {
#include "traverse_leaf.inc"
            cur = kInvalidRef;
        } else if constexpr (!SS) {
            // ---- TLAS leaf: enter the first instance, keep the rest of the list on the stack
            const uint32_t first = cur & kLeafFirstMask, count = ((cur >> 27) & 15u) + 1u;
            if (count > 1) push(make_leaf(first + 1, count - 1));
            const uint32_t gid = sc.tlas_prims[first];
            const float4* ip = reinterpret_cast<const float4*>(sc.instances + gid);
            const uint4 meta = *reinterpret_cast<const uint4*>(ip + 3);
            if (COUNT) tc.insts++;
            if (meta.z & kInstanceIdentity) {
                // an instance whose inverse is exactly the identity (k_prepare_instances): the matrix product below is v * 1 + 0 + 0 + 0 per
                // component = v + 0.0f (a -0 becomes +0 as it does there); o, d ARE the world ray here (a TLAS leaf is reached in world space)
                o = mk3(o.x + 0.0f, o.y + 0.0f, o.z + 0.0f);
                d = mk3(d.x + 0.0f, d.y + 0.0f, d.z + 0.0f);
            } else {
                const float4 r0 = ip[0], r1 = ip[1], r2 = ip[2];
                // ray into object space with the inverse instance matrix; direction NOT renormalised (ray_gen.comp:340-341)
                o = xform_rows(r0, r1, r2, world_o(), 1.0f);
                d = xform_rows(r0, r1, r2, world_d(), 0.0f);
            }
            inv = slab_inv(d);
            tri_base = meta.y;
            cur_inst = (int32_t)gid;
            nodes = space_nodes(sc, true, meta.x, inv);
            blas_sp = sp;
            cur = 0;
            continue;
        }
        // ---- next entry
        if (!SS && blas_sp >= 0 && sp == blas_sp) { // BLAS exhausted: back to world space
            blas_sp = -1;
            o = world_o();
            d = world_d();
            inv = slab_inv(d);
            nodes = space_nodes(sc, false, 0u, inv);
        }
        if (sp == 0) { RFW_TRAV_EXHAUSTED }
        cur = pop();
    }
