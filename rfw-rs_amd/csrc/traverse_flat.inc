// traverse_flat.inc — the FLAT traversal loop of traverse.h: plain any hit and both streaming kinds.
// Hooks: RFW_TRAV_TOP (start of every trip: the streaming kernels' supply of rays), RFW_TRAV_OCCLUDED (traverse_leaf.inc), RFW_TRAV_FLAT_WHILE (the
// loop's wave-uniform condition), RFW_TRAV_LEAF_TRIP / RFW_TRAV_TLAS_TRIP (wave-uniform: leaves / instance lists are worked on in this trip).
// No hook may `continue`.
    uint32_t iteration = 0;
    // The loop WITHOUT else-branches, `continue` or a divergent way out: every stage of a
    // trip — node test, leaf, instance list, change of space, next stack entry — is an `if` of its own, and what a lane does next is told by
    // `cur` alone: an interior reference, a leaf reference, kInvalidRef ("take the next stack entry") or kDoneRef ("finished": the lane stays
    // in the loop, switched off, until the wavefront has no unfinished lane — one scalar test).  The same work per lane and trip as the
    // nested form below.  What goes away is mask arithmetic: a flag that lives across divergent branches is an SGPR pair the compiler
    // merges with three scalar instructions at every join, and an if / else-if / else chain with two `continue`s and two exits needs a
    // dozen of them per trip — a third of the instructions of a trip, in a loop bound by instruction issue.  Here every carried value is a
    // vector register written under the branch's own exec mask.
    constexpr uint32_t kDoneRef = 0xfffffffeu, kIdleRef = 0xfffffffdu; // (like kInvalidRef not leaves that can exist: first + count <= 2^27 - 1)
    // kDoneRef: the lane's ray is finished (streaming: waiting to be committed); kIdleRef (streaming only): the lane holds no ray at all
    uint32_t occ_ = 0u;
    while (RFW_TRAV_FLAT_WHILE) {
        iteration++;
        RFW_TRAV_TOP
        uint32_t enter_gid = kInvalidRef;
        const bool leaf_trip_ = RFW_TRAV_LEAF_TRIP, tlas_trip_ = RFW_TRAV_TLAS_TRIP; // (wave-uniform)
        if ((int32_t)cur >= 0) {
#include "traverse_node.inc"
        }
        if (leaf_trip_ && (((int32_t)cur < -3) & (SS || blas_sp >= 0))) {
            uint32_t next_ = kInvalidRef;
#include "traverse_leaf.inc"
            cur = next_;
        }
        if constexpr (!SS) if (tlas_trip_ && (((int32_t)cur < -3) & (blas_sp < 0))) {
            // ---- TLAS leaf: the first instance is entered below, the rest of the list stays on the stack
            const uint32_t first = cur & kLeafFirstMask, count = ((cur >> 27) & 15u) + 1u;
            if (count > 1) push(make_leaf(first + 1, count - 1));
            enter_gid = sc.tlas_prims[first];
            if (COUNT) tc.insts++;
        }
        // ---- a change of space (into the instance just found / back to the world when its tree is exhausted) happens in ONE place: the ray,
        // its reciprocal and the node array have a single definition per trip (two made the compiler carry a second copy of all of them
        // around the loop: 24 v_mov per trip)
        if constexpr (SS) { // one space: nothing to enter or leave, only the next stack entry
            const bool next_entry_ = cur == kInvalidRef, last_ = next_entry_ & (sp == 0);
            if (next_entry_ & !last_) cur = pop();
            cur = last_ ? kDoneRef : cur;
        } else {
            const bool enter = enter_gid != kInvalidRef;
            const bool leave = (cur == kInvalidRef) & (blas_sp >= 0) & (sp == blas_sp);
            if (enter | leave) {
                uint32_t node_base = 0;
                if (enter) {
                    const float4* ip = reinterpret_cast<const float4*>(sc.instances + enter_gid);
                    const uint4 meta = *reinterpret_cast<const uint4*>(ip + 3);
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
                    tri_base = meta.y;
                    cur_inst = (int32_t)enter_gid;
                    node_base = meta.x;
                } else {
                    o = world_o();
                    d = world_d();
                }
                blas_sp = enter ? sp : -1;
                inv = slab_inv(d);
                nodes = space_nodes(sc, enter, node_base, inv);
            }
            if (enter) cur = 0;
            const bool next_entry_ = cur == kInvalidRef, last_ = next_entry_ & (sp == 0); // (last_: the lane's stack is empty, its ray is done)
            if (next_entry_ & !last_) cur = pop();
            cur = last_ ? kDoneRef : cur;
        }
    }
