// api_frame.cpp — instance life cycle and the per-frame launch sequence of the C ABI (backends/gpu-rt/src/lib.rs:1685-1780 render): frame slots,
// batches, samples, reads and downloads, options, timing.
#include "api_internal.h"

using namespace rfwapi;

namespace rfwapi {
thread_local std::string g_create_error;
} // namespace rfwapi
namespace rfwhip {
static EnvSwitches g_env;
const EnvSwitches& env_switches() { return g_env; }
void read_env_switches()
{
    EnvSwitches e;
    auto set = [](const char* name) { const char* v = getenv(name); return v != nullptr && std::strcmp(v, "0") != 0; };
    e.build_trace = set("RFW_BUILD_TRACE");
    e.no_forest = set("RFW_NO_FOREST");
    e.lbvh_fenced = set("RFW_LBVH_FENCED");
    e.p2p_data_cached = set("RFW_P2P_DATA_CACHED");
    e.p2p_flags_finegrained = set("RFW_P2P_FLAGS_FINEGRAINED");
    if (const char* v = getenv("RFW_PACKET_AUTO_MAX_TRIANGLES")) e.packet_auto_max_triangles = strtoull(v, nullptr, 10);
    if (const char* v = getenv("RFW_SPATIAL_SPLITS")) { e.has_spatial_splits = true; e.spatial_splits = (float)std::max(0.0, atof(v)); }
    if (const char* v = getenv("RFW_PACKET_TRACE")) e.packet_trace = std::max(0, atoi(v));
    static std::mutex mu; // (instances may be created from several threads)
    std::lock_guard<std::mutex> g(mu);
    g_env = e;
}
} // namespace rfwhip
namespace rfwapi {
// m with n / d == (n * m) >> 32 for every n <= n_max, or 0 when the round-up reciprocal m = ceil(2^32 / d) is not exact that far
// (n * m = n * 2^32 / d + n * e / d with e = m * d - 2^32 < d: exact while n_max * e < 2^32).  The kernels divide when they get 0.
uint32_t index_magic(const uint32_t d, const uint64_t n_max)
{
    if (d < 2u) return 0u;
    const uint64_t m = ((1ull << 32) + d - 1u) / d, e = m * d - (1ull << 32);
    if (m > 0xffffffffull || n_max >= (1ull << 32)) return 0u;
    return (e == 0 || n_max < (1ull << 32) / e) ? (uint32_t)m : 0u;
}

void compute_shard(Instance* I)
{
    // virtual sharding: world x substreams virtual ranks; virtual rank rank*S + s belongs to this instance's sub-shard s
    const uint32_t S = I->substreams, wv = I->world * S;
    I->tiles_x = (I->width + I->tile_size - 1) / I->tile_size;
    I->tiles_y = (I->height + I->tile_size - 1) / I->tile_size;
    const uint32_t total = I->tiles_x * I->tiles_y;
    I->local_tiles_v = (total + wv - 1) / wv; // every sub-slab is padded to the same size on every rank
    I->cap_v = I->local_tiles_v * I->tile_size * I->tile_size;
    I->local_tiles = I->local_tiles_v * S;
    I->capacity = I->cap_v * S;
    uint64_t px = 0;
    for (uint32_t t = 0; t < total; t++) {
        if ((t % wv) / S != I->rank) continue;
        const uint32_t tx = t % I->tiles_x, ty = t / I->tiles_x;
        const uint32_t w = std::min(I->tile_size, I->width - tx * I->tile_size), h = std::min(I->tile_size, I->height - ty * I->tile_size);
        px += (uint64_t)w * h;
    }
    I->local_pixels = px;
}

int alloc_paths(Instance* I)
{
    compute_shard(I);
    const size_t n = (size_t)I->capacity * I->max_batch; // a batch of frames is one tall virtual frame
    for (int h = 0; h < 2; h++) {
        HIP_TRY(I, I->d_ray_o[h].ensure(n));
        HIP_TRY(I, I->d_ray_d[h].ensure(n));
        HIP_TRY(I, I->d_thr[h].ensure(n));
        HIP_TRY(I, I->d_hit[h].ensure(n));
    }
    HIP_TRY(I, I->d_sh_o.ensure(n * kShadowBuckets));
    HIP_TRY(I, I->d_sh_d.ensure(n * kShadowBuckets));
    HIP_TRY(I, I->d_sh_e.ensure(n * kShadowBuckets));
    HIP_TRY(I, I->d_acc_slab.ensure(n));
    HIP_TRY(I, hipMemsetAsync(I->d_acc_slab.ptr, 0, n * sizeof(float4), I->stream));
    const size_t px = (size_t)I->width * I->height * I->max_batch;
    HIP_TRY(I, I->d_frame_out.ensure(px));
    I->acc_source = nullptr;
    HIP_TRY(I, hipMemsetAsync(I->d_frame_out.ptr, 0, px * sizeof(float4), I->stream));
    if (scaled(I)) { // the window frame (zeros until the first render); the same-size path has none
        const size_t wpx = (size_t)I->window_w * I->window_h * I->max_batch;
        HIP_TRY(I, I->d_frame_win.ensure(wpx));
        HIP_TRY(I, hipMemsetAsync(I->d_frame_win.ptr, 0, wpx * sizeof(float4), I->stream));
    } else I->d_frame_win.release();
    // per-thread overflow slots: launch grids are padded (XCD tiling, shadow buckets), so leave a margin per sub-shard
    HIP_TRY(I, I->d_spill.ensure((size_t)kStackSpill * I->substreams * ((size_t)I->cap_v * I->max_batch + kSpillMargin)));
    HIP_TRY(I, I->d_counters.ensure(2 * kMaxSub));
    HIP_TRY(I, hipMemsetAsync(I->d_counters.ptr, 0, 2 * kMaxSub * sizeof(QueueCounters), I->stream));
    I->sample_count = 0;
    I->ao_rounds = 0; // (the shadow queue was reallocated: no AO rays to report)
    return RFW_HIP_OK;
}

uint32_t spill_stride(const Instance* I) { return (uint32_t)(I->d_spill.cap / kStackSpill); }

SceneDev scene_dev(Instance* I)
{
    SceneDev s;
    const Instance* S = scene_of(I); // a frame slot reads its owner's scene
    const Instance* TL = tlas_of(I);
    s.tlas_nodes = TL->d_tlas_nodes.ptr;
    s.tlas_prims = TL->d_tlas_prims.ptr;
    s.instances = TL->d_xforms.ptr;
    s.instance_normals = TL->d_normals.ptr;
    s.meshes = S->d_mesh_records.ptr;
    s.tlas_wide = TL->d_tlas_wide.ptr;
    s.blas_wide = S->d_blas_wide.ptr;
    s.tlas_wide_stride = (uint32_t)(TL->d_tlas_oct.cap / kPacketNodeCopies); // (both forms of the copies share the stride; the packet form may be absent)
    s.blas_wide_stride = (uint32_t)(S->d_blas_oct.cap / kPacketNodeCopies);
    s.tlas_oct = TL->d_tlas_oct.ptr;
    s.blas_oct = S->d_blas_oct.ptr;
    s.blas_oct_abs = S->d_blas_oct_abs.ptr;
    s.ss_root = (S->single_space_opt != 0 && TL->ss_ready && S->d_blas_oct_abs.ptr) ? TL->ss_root : 0u; // (TL's TLAS and graft are of one instances_version; a graft's root is never node 0)
    s.tri_packets = S->d_packets.ptr;
    s.triangles = S->d_triangles.ptr;
    const Instance::Tables& tb = S->tables[S->tables_version % Instance::kTableVersions];
    s.materials = tb.materials.ptr;
    s.area_lights = tb.area.ptr;
    s.point_lights = tb.point.ptr;
    s.spot_lights = tb.spot.ptr;
    s.directional_lights = tb.dir.ptr;
    s.tex_data = S->d_tex_data.ptr;
    s.tex_desc = S->d_tex_desc.ptr;
    s.n_textures = S->n_textures;
    s.skybox = S->skybox_desc;
    s.blue_noise = S->has_blue_noise ? S->d_blue_noise.ptr : nullptr;
    s.spill = I->d_spill.ptr;
    s.spill_stride = spill_stride(I);
    s.spill_rows = std::min<uint32_t>(scene_of(I)->spill_rows, (uint32_t)kStackSpill);
    s.overflow_flag = I->overflow_dev;
    s.counters = I->d_counters.ptr + (size_t)I->counter_phase * kMaxSub; // (the latest frame's block)
    s.counters_next = nullptr;
    return s;
}

CameraParams camera_params(const Instance* I, const rfw_camera_view_3d& v, uint32_t sub)
{
    CameraParams c;
    std::memset(&c, 0, sizeof(c));
    c.pos[0] = v.pos.x; c.pos[1] = v.pos.y; c.pos[2] = v.pos.z;
    c.lens_size = v.lens_size;
    c.right[0] = v.right.x; c.right[1] = v.right.y; c.right[2] = v.right.z;
    c.spread_angle = v.spread_angle;
    c.up[0] = v.up.x; c.up[1] = v.up.y; c.up[2] = v.up.z;
    c.clamp_value = I->clamp_value;
    c.p1[0] = v.p1.x; c.p1[1] = v.p1.y; c.p1[2] = v.p1.z;
    c.width = I->width; c.height = I->height;
    c.sample_count = I->image_offset + I->sample_count; // the sample's INDEX (seeds, blue noise); the finalisers get the count I->sample_count
    const Instance* S = scene_of(I);
    c.point_light_count = (uint32_t)S->point_lights.size();
    c.area_light_count = (uint32_t)S->area_lights.size();
    c.spot_light_count = (uint32_t)S->spot_lights.size();
    c.directional_light_count = (uint32_t)S->directional_lights.size();
    c.tile_size = I->tile_size; c.tiles_x = I->tiles_x; c.tiles_y = I->tiles_y;
    c.rank = I->rank * I->substreams + sub; c.world = I->world * I->substreams; c.local_tiles = I->local_tiles_v;
    c.flags = I->flags;
    c.tile_shift = (I->tile_size & (I->tile_size - 1u)) == 0u ? (uint32_t)__builtin_ctz(I->tile_size) : 0xffffffffu;
    c.width_magic = index_magic(I->width, (uint64_t)I->width * I->height);
    // (slab indices run a little past the last tile: idx < capacity of the rank's slab, tile = lt * world + rank)
    c.tiles_x_magic = index_magic(I->tiles_x, (uint64_t)I->tiles_x * I->tiles_y + 4096ull * std::max<uint64_t>((uint64_t)I->world * I->substreams, 1ull));
    // (api_internal.h: far outside the caches one ray per lane wins)
    if (S->packet_auto && S->n_tris > packet_auto_limit()) c.flags &= ~kFlagPacketPrimary;
    c.max_path_length = I->max_path_length;
    c.sky[0] = I->sky[0]; c.sky[1] = I->sky[1]; c.sky[2] = I->sky[2];
    c.batch = 1;
    // streaming trades the tail of every wavefront for fewer, longer wavefronts: it pays when other frames fill the chip meanwhile (measured on
    // C4 path traced: 8 frame slots 2880 -> 3190 Mrays/s, 4 slots 2840 -> 3100; but 2 slots 2770 -> 2610, one frame at a time 2270 -> 1670,
    // and batches, whose extension rays are traced in sorted order, 3480 -> 3360).  Unless the option was set by hand it is on for single
    // frames of an instance with four or more frame slots (and for batches, which fill the chip by themselves: do_render)
    const Instance* S_ = scene_of(I);
    c.stream_run = (S_->stream_auto && !(S_->slots.size() + 1 >= 4)) ? 0u : S_->stream_run;
    c.stream_refill = std::max(1u, std::min(64u, scene_of(I)->stream_refill)) | (std::max(1u, std::min(64u, scene_of(I)->stream_leaf_gate)) << 8);
    c.frame_capacity = I->cap_v;
    return c;
}

PathDev path_dev(Instance* I, uint32_t sub)
{
    PathDev p;
    const size_t off = (size_t)sub * I->cap_v;
    for (int h = 0; h < 2; h++) {
        p.ray_o[h] = I->d_ray_o[h].ptr + off;
        p.ray_d[h] = I->d_ray_d[h].ptr + off;
        p.thr[h] = I->d_thr[h].ptr + off;
        p.hit[h] = I->d_hit[h].ptr + off;
    }
    p.sh_o = I->d_sh_o.ptr + off * kShadowBuckets;
    p.sh_d = I->d_sh_d.ptr + off * kShadowBuckets;
    p.sh_e = I->d_sh_e.ptr + off * kShadowBuckets;
    p.acc = I->d_acc_slab.ptr + off;
    p.capacity = I->cap_v;
    return p;
}

inline int ev_index(uint32_t bounce, int kernel, int end) { return EV_KERNEL_BASE + 2 * ((int)bounce * kKernelsPerBounce + kernel) + end; }
constexpr int kEvBlit = EV_KERNEL_BASE + 2 * (kMaxBounces * kKernelsPerBounce);

hipEvent_t* ring_events(Instance* I, int slot, uint32_t sub) { return I->ring.data() + ((size_t)slot * I->substreams + sub) * kNumEvents; }

// option "ao_radius" = 0: 5 % of the diagonal of the world bounds of the scene's instances (mesh boxes as handed over, through the instance
// matrices), on the host, once per scene version — at the first ambient occlusion frame after a synchronize() that changed the scene
static float ao_radius_of(Instance* I)
{
    if (I->ao_radius > 0.0f) return I->ao_radius;
    Instance* O = scene_of(I);
    if (O->ao_auto_version != O->scene_version) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (const auto& kv : O->inst_lists) {
            const rfw_aabb& b = kv.second.local_aabb;
            for (const rfw_mat4& m : kv.second.matrices) {
                bool zero = true;
                for (int c = 0; c < 16; c++) zero = zero && m.m[c] == 0.0f;
                if (zero) continue; // a removed slot
                for (int c = 0; c < 8; c++) {
                    const float x = (c & 1) ? b.max[0] : b.min[0], y = (c & 2) ? b.max[1] : b.min[1], z = (c & 4) ? b.max[2] : b.min[2];
                    const float w[3] = {m.m[0] * x + m.m[4] * y + m.m[8] * z + m.m[12], m.m[1] * x + m.m[5] * y + m.m[9] * z + m.m[13],
                                        m.m[2] * x + m.m[6] * y + m.m[10] * z + m.m[14]};
                    for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], w[a]); hi[a] = std::max(hi[a], w[a]); }
                }
            }
        }
        double d2 = 0.0;
        for (int a = 0; a < 3; a++) d2 += hi[a] >= lo[a] ? ((double)hi[a] - lo[a]) * ((double)hi[a] - lo[a]) : 0.0;
        O->ao_auto_radius = d2 > 0.0 ? (float)(0.05 * std::sqrt(d2)) : 1.0f;
        O->ao_auto_version = O->scene_version;
    }
    return O->ao_auto_radius;
}

int do_render(Instance* I, const rfw_camera_view_3d* views, uint32_t k, bool samples, uint32_t mode)
{
    const rfw_camera_view_3d& view = views[0];
    HIP_TRY(I, hipSetDevice(I->device));
    if (!scene_of(I)->synchronized || tlas_of(I)->d_tlas_nodes.ptr == nullptr) return RFW_HIP_OK; // render before any mesh exists (gpu-rt/src/lib.rs:1686-1688)
    if (I->scene && I->scene->scene_ready && I->waited_version != I->scene->scene_version) { // a slot must not read a scene still being written
        HIP_TRY(I, hipStreamWaitEvent(I->stream, I->scene->scene_ready, 0));
        I->waited_version = I->scene->scene_version;
    }
    {   // the material / light tables this frame reads: wait (on the device) for their upload, once per version
        Instance* S = scene_of(I);
        if (S->tables_ready && I->tables_waited != S->tables_version) {
            HIP_TRY(I, hipStreamWaitEvent(I->stream, S->tables_ready, 0));
            I->tables_waited = S->tables_version;
        }
        I->tables_used = S->tables_version;
        if (I->tables_oldest_pending == ~0ull) I->tables_oldest_pending = S->tables_version;
    }
    if ((I->have_last_view && (std::memcmp(&I->last_view, &view, sizeof(view)) != 0 || mode != I->render_mode)) || I->after_batch) I->sample_count = 0;
    I->render_mode = mode; // (a change of mode starts a new image, as a change of view does)
    I->after_batch = k > 1 && !samples; // the frames of a batch are complete images: whatever follows starts a new one
    I->last_view = view;
    I->have_last_view = true;
    if (k > 1) {
        if (k > I->max_batch || k > (uint32_t)kMaxBatch) return fail(I, RFW_HIP_E_INVALID, "render_batch: more frames than options.max_batch");
        if (I->substreams > 1) return fail(I, RFW_HIP_E_STATE, "render_batch: not available with sub-streams");
        // the frame index rides in bits 24..31 of the path word, next to the PIXEL index of the whole frame (not of this rank's slab)
        if ((uint64_t)I->width * I->height >= (1ull << 24)) return fail(I, RFW_HIP_E_INVALID, "render_batch: frames of 2^24 pixels or more cannot be batched");
        for (uint32_t f = 1; f < k; f++)
            if (views[f].spread_angle != view.spread_angle) return fail(I, RFW_HIP_E_INVALID, "render_batch: the views of a batch must share one spread angle (field of view and height)");
        if (!samples) I->sample_count = 0; // every frame of a batch is a new image
    }

    const uint32_t S = I->substreams;
    const bool count = (I->flags & RFW_HIP_FLAG_COUNT_TRAVERSAL) != 0;
    const bool nee = !(I->flags & RFW_HIP_FLAG_NO_NEE);
    hipStream_t main = I->stream;
    const bool tm = I->timing;
    const int slot = (int)(I->frame_index % kTimingRing);
    I->events = ring_events(I, slot, 0);
    const uint32_t bounces = std::min<uint32_t>(I->max_path_length, kMaxBounces);
    const bool ao = mode >= RFW_HIP_RENDER_SSAO;
    const uint32_t ao_rounds = ao ? I->ao_samples : 0u;
    if (ao) HIP_TRY(I, I->d_ao_guide.ensure((size_t)I->width * I->height));
    // option "denoise": the a-trous filter finalises the path-traced frame where launch_assemble would (the frame is de-tiled on this device
    // and the call leaves ONE image behind); everywhere else the option changes nothing
    const bool dn = I->denoise > 0 && mode == RFW_HIP_RENDER_DEFAULT && (k == 1 || samples) && I->world <= 1 && !scene_of(I)->comm && !scene_of(I)->loop &&
                    !scene_of(I)->p2p.connected;
    if (dn) {
        const size_t px = (size_t)I->width * I->height;
        HIP_TRY(I, I->d_dn_guide.ensure(3 * px));
        for (int q = 0; q < 2 && I->denoise > 1; q++) HIP_TRY(I, I->d_dn_plane[q].ensure(px));
    }
    // option "denoise_temporal": acts where the filter does.  Option "sample_offset": where an image starts, its first sample index is fixed
    // (a batch of frames keeps index 0); the kernels clear the accumulator at index 0 only, so an image that starts elsewhere is cleared here
    Instance* const O = scene_of(I);
    const bool dnt = dn && O->denoise_temporal > 0;
    const bool new_image = I->sample_count == 0;
    if (new_image) {
        I->image_offset = (k > 1 && !samples) ? 0u : O->sample_offset;
        if (dnt) {
            I->dn_image = O->dn_images++;
            I->image_offset += I->dn_image & 255u;
        }
    }
    if (dnt) {
        const size_t px = (size_t)I->width * I->height;
        for (int q = 0; q < 2; q++) HIP_TRY(I, O->d_dn_history[q].ensure(3 * px));
        if (!O->dn_chain) HIP_TRY(I, hipEventCreateWithFlags(&O->dn_chain, hipEventDisableTiming));
    }
    // option "tonemap": the display transform acts on the finished frame of a path-traced image where the frame is de-tiled on this device
    // and the call leaves ONE image behind (as "denoise"); off: no launch, no allocation
    const bool disp = O->display.curve > 0 && mode == RFW_HIP_RENDER_DEFAULT && (k == 1 || samples) && I->world <= 1 && !O->comm && !O->loop && !O->p2p.connected;
    // option "denoise_motion": acts where the temporal option does
    const bool dnm = dnt && O->denoise_motion > 0;
    if (dnm) {
        const size_t px = (size_t)I->width * I->height;
        HIP_TRY(I, I->d_dn_ids.ensure(px));
        for (int q = 0; q < 2; q++) HIP_TRY(I, O->d_dn_history_ids[q].ensure(px));
    }
    // option "denoise_deform": acts where the motion option does
    const bool dnd = dnm && O->denoise_deform > 0;
    if (dnd) HIP_TRY(I, I->d_dn_tris.ensure((size_t)I->width * I->height));

    // The 2D layer: where the frame is de-tiled on this device and the call leaves one image of rfw_hip_render behind, the draws of the last
    // synchronize() go over the finalised frame.  Nothing to draw, or no view_2d: no launch, no allocation, no wait.
    const Instance::OvVersion* ov = nullptr;
    I->ov_frame_prims = I->ov_frame_words = 0;
    if (O->view_2d && k == 1 && !samples && I->world <= 1 && !O->comm && !O->loop && !O->p2p.connected && !I->external_slab) {
        const Instance::OvVersion& v = O->ov[O->ov_version % Instance::kTableVersions];
        if (v.n_prims) {
            ov = &v;
            if (I->ov_waited != O->ov_version) {
                HIP_TRY(I, hipStreamWaitEvent(main, O->ov_ready, 0));
                I->ov_waited = O->ov_version;
            }
            if (I->ov_oldest_pending == ~0ull) I->ov_oldest_pending = O->ov_version;
        }
    }

    if (tm) (void)hipEventRecord(I->events[EV_FRAME0], main);
    // queue counters: this frame takes the block the previous frame's k_primary cleared (alloc_paths cleared both), and clears the other
    I->counter_phase ^= 1u;
    // The frame's tiles are dealt to S sub-shards, each with its own queues, counters and accumulator slab, each traced on its
    // own stream: the long tail of one sub-shard's trace kernel (the slowest wavefront bounds a launch) overlaps the other
    // sub-shards' kernels.  Fork from / join into the caller's stream with events.
    if (S > 1) HIP_TRY(I, hipEventRecord(I->ev_fork, main));
    SceneDev sc[kMaxSub];
    PathDev p[kMaxSub];
    CameraParams cam[kMaxSub];
    hipStream_t st[kMaxSub];
    for (uint32_t s = 0; s < S; s++) {
        st[s] = S > 1 ? I->sub[s] : main;
        if (S > 1) HIP_TRY(I, hipStreamWaitEvent(st[s], I->ev_fork, 0));
        sc[s] = scene_dev(I);
        sc[s].counters = I->d_counters.ptr + (size_t)I->counter_phase * kMaxSub + s;
        sc[s].counters_next = I->d_counters.ptr + (size_t)(I->counter_phase ^ 1u) * kMaxSub + s;
        sc[s].spill = I->d_spill.ptr + (size_t)s * (I->cap_v + kSpillMargin);
        p[s] = path_dev(I, s);
        cam[s] = camera_params(I, view, s);
        if (new_image && I->image_offset != 0u) HIP_TRY(I, hipMemsetAsync(p[s].acc, 0, (size_t)I->cap_v * sizeof(float4), st[s]));
        {   // k_shade's workgroup size (kernels.hip, k_shade): small where other frames' kernels share the chip with this call
            const Instance* O = scene_of(I);
            const int g = O->shade_group;
            if (g == 256 || (g == 0 && k == 1 && !O->slots.empty())) cam[s].flags |= kFlagShadeSmallGroups;
            // option "material_maps": k_shade_maps in k_shade's place only where the table this frame reads holds a parameter map
            if (O->material_maps && O->mat_param_maps) cam[s].flags |= kFlagMaterialMaps;
        }
    }
    BatchViews bv;
    if (k > 1) {
        cam[0].batch = k;
        // a batch fills the chip by itself: its bounces stream whatever the number of frame slots (and are then NOT sorted, see below)
        if (scene_of(I)->stream_auto) cam[0].stream_run = scene_of(I)->stream_run;
        p[0].capacity = I->cap_v * k;
        for (uint32_t f = 0; f < k; f++) {
            cam[0].batch_sample[f] = samples ? I->image_offset + I->sample_count + f : 0u;
            FrameView& v = bv.v[f];
            v.pos[0] = views[f].pos.x; v.pos[1] = views[f].pos.y; v.pos[2] = views[f].pos.z; v.lens_size = views[f].lens_size;
            v.right[0] = views[f].right.x; v.right[1] = views[f].right.y; v.right[2] = views[f].right.z; v.pad0 = 0.0f;
            v.up[0] = views[f].up.x; v.up[1] = views[f].up.y; v.up[2] = views[f].up.z; v.pad1 = 0.0f;
            v.p1[0] = views[f].p1.x; v.p1[1] = views[f].p1.y; v.p1[2] = views[f].p1.z; v.pad2 = 0.0f;
        }
    }
    if (mode != RFW_HIP_RENDER_DEFAULT) {
        // render modes 1-6 (aov.inc): the camera rays of mode 0, then the mode's value at their hits — or the ambient occlusion rays, traced
        // through the shadow queue one round per launch (k_shadow adds to the accumulator with one writer per slot and launch)
        const float radius = ao ? ao_radius_of(I) : 0.0f;
        const float dir[3] = {view.direction.x, view.direction.y, view.direction.z};
        for (uint32_t s = 0; s < S; s++) {
            hipEvent_t* ev = ring_events(I, slot, s);
            if (tm) (void)hipEventRecord(ev[ev_index(0, 0, 0)], st[s]);
            launch_primary(st[s], cam[s], sc[s], p[s], count);
            if (tm) (void)hipEventRecord(ev[ev_index(0, 0, 1)], st[s]);
            if (tm) (void)hipEventRecord(ev[ev_index(0, 1, 0)], st[s]);
            launch_aov(st[s], cam[s], sc[s], p[s], mode, ao_rounds, radius, I->d_ao_guide.ptr, dir);
            if (tm) (void)hipEventRecord(ev[ev_index(0, 1, 1)], st[s]);
            if (tm) (void)hipEventRecord(ev[ev_index(0, 2, 0)], st[s]);
        }
        for (uint32_t r = 0; r < ao_rounds; r++)
            for (uint32_t s = 0; s < S; s++) launch_shadow(st[s], cam[s], sc[s], p[s], r, count);
        for (uint32_t s = 0; s < S; s++)
            if (tm) (void)hipEventRecord(ring_events(I, slot, s)[ev_index(0, 2, 1)], st[s]);
    }
    for (uint32_t b = 0; b < bounces && mode == RFW_HIP_RENDER_DEFAULT; b++) { // gpu-rt/src/lib.rs:1708-1728 without the read-back; stage by stage across the sub-shards
        for (uint32_t s = 0; s < S; s++) {
            hipEvent_t* ev = ring_events(I, slot, s);
            if (tm) (void)hipEventRecord(ev[ev_index(b, 0, 0)], st[s]);
            if (b == 0 && k > 1) launch_primary_batch(st[s], cam[s], bv, sc[s], p[s], count);
            else if (b == 0) launch_primary(st[s], cam[s], sc[s], p[s], count);
            else {
                const uint32_t* order = nullptr;
                // Measured on C4, max path length 3 (EXPERIMENTS.md): a single 1-spp frame has too few rays per cell and direction for the sort
                // to form coherent wavefronts (+1.5 % with frames in flight, -2.7 % alone: it costs a 2 M-pair sort per bounce); a batch of 8
                // frames — or k samples of one image — sorts 8 x / k x as many rays of the same surfaces together: +17 %
                // Round 3: streaming (traverse_stream) does for a batch what the sort does, without the sort — batches of 8: 3480 sorted, 3490
                // streaming, 3300 both; 4 samples of one image per call: 3070 sorted, 3415 streaming, 3130 both — so "only where it pays"
                // (mode 2) now means: batches whose bounces do NOT stream
                const int mode = scene_of(I)->sort_extension_rays;
                if ((mode == 1 || (mode == 2 && k > 1 && cam[s].stream_run == 0u)) && S == 1) { // (sub-shards keep the queue order: one sort buffer per instance)
                    const size_t n = p[s].capacity;
                    for (int q = 0; q < 2; q++) { HIP_TRY(I, I->d_sort_keys[q].ensure(n)); HIP_TRY(I, I->d_sort_vals[q].ensure(n)); }
                    HIP_TRY(I, I->d_sort_ws.ensure(sort_pairs_workspace_bytes((uint32_t)n)));
                    launch_extension_keys(st[s], sc[s], p[s], b, I->d_sort_keys[0].ptr, I->d_sort_vals[0].ptr);
                    HIP_TRY(I, sort_pairs_u32(st[s], I->d_sort_ws.ptr, I->d_sort_ws.cap, I->d_sort_keys[0].ptr, I->d_sort_keys[1].ptr, I->d_sort_vals[0].ptr,
                                              I->d_sort_vals[1].ptr, (uint32_t)n, 32));
                    order = I->d_sort_vals[1].ptr;
                }
                launch_extend(st[s], cam[s], sc[s], p[s], b, count, order);
            }
            if (tm) (void)hipEventRecord(ev[ev_index(b, 0, 1)], st[s]);
            if (b == 0 && dn) { // the filter's guide, before k_shade and bounce 2 reuse the [0] buffers; of k samples, the LAST one's
                PathDev g = p[s];
                if (k > 1) {
                    const size_t last = (size_t)(k - 1u) * I->cap_v;
                    g.hit[0] += last; g.ray_o[0] += last; g.ray_d[0] += last;
                    g.capacity = I->cap_v;
                }
                launch_dn_guide(st[s], cam[s], sc[s], g, I->d_dn_guide.ptr, k > 1 ? 0x00ffffffu : 0xffffffffu);
                if (dnm) launch_dn_ids(st[s], cam[s], g, I->d_dn_ids.ptr, k > 1 ? 0x00ffffffu : 0xffffffffu);
                if (dnd) launch_dn_tris(st[s], cam[s], sc[s], g, I->d_dn_tris.ptr, k > 1 ? 0x00ffffffu : 0xffffffffu);
            }
        }
        for (uint32_t s = 0; s < S; s++) {
            hipEvent_t* ev = ring_events(I, slot, s);
            if (tm) (void)hipEventRecord(ev[ev_index(b, 1, 0)], st[s]);
            launch_shade(st[s], cam[s], sc[s], p[s], b);
            if (tm) (void)hipEventRecord(ev[ev_index(b, 1, 1)], st[s]);
        }
        if (nee)
            for (uint32_t s = 0; s < S; s++) {
                hipEvent_t* ev = ring_events(I, slot, s);
                if (tm) (void)hipEventRecord(ev[ev_index(b, 2, 0)], st[s]);
                launch_shadow(st[s], cam[s], sc[s], p[s], b, count);
                if (tm) (void)hipEventRecord(ev[ev_index(b, 2, 1)], st[s]);
            }
    }
    if (S > 1)
        for (uint32_t s = 0; s < S; s++) {
            HIP_TRY(I, hipEventRecord(I->ev_join[s], st[s]));
            HIP_TRY(I, hipStreamWaitEvent(main, I->ev_join[s], 0));
        }
    if (samples && k > 1) { // the k sample slabs -> the image's accumulator (slab 0), in sample order
        launch_sum_batch(main, I->d_acc_slab.ptr, I->cap_v, k);
        cam[0].batch = 1;
    }
    I->sample_count += samples ? k : 1;
    const uint32_t frames_out = samples ? 1u : k; // images this call leaves behind
    if (tm) (void)hipEventRecord(I->events[kEvBlit], main);
    if (Instance* C = scene_of(I); C->comm || C->loop) {
        // the frame's ONE collective, issued by the library itself: this rank's slab(s) -> all ranks (RCCL over xGMI) -> de-tile
        const uint64_t n_send = slab_words(I) * frames_out; // 4-byte words, whatever they hold
        pack_slabs(I, main, I->d_send.ptr, frames_out);
        if (C->comm_chain && C->comm_chain_pending) HIP_TRY(I, hipStreamWaitEvent(main, C->comm_chain, 0)); // behind the previous slot's collective
        if (C->loop) { // (the test transport: same buffers, same ordering around it)
            const int lrc = loop_all_gather(I, main, n_send);
            if (lrc != RFW_HIP_OK) return lrc;
        } else {
            const ncclResult_t nr = g_rccl.all_gather(I->d_send.ptr, I->d_recv.ptr, n_send, ncclFloat, C->comm, main);
            if (nr != ncclSuccess) return fail(I, RFW_HIP_E_DEVICE, std::string("ncclAllGather: ") + g_rccl.error_string(nr));
        }
        if (C->comm_chain) { HIP_TRY(I, hipEventRecord(C->comm_chain, main)); C->comm_chain_pending = true; }
        const int arc = gathered_arrived(I, main, I->d_recv.ptr, frames_out); // gathered = [rank][frame][slab]
        if (arc != RFW_HIP_OK) return arc;
    } else if (C->p2p.connected) {
        const int prc = p2p_exchange(I, main, frames_out);
        if (prc != RFW_HIP_OK) return prc;
    } else if (I->world <= 1) // de-tile the sub-slabs into the linear accumulator / tonemapped frame (blit.comp:15-23)
    {
        if (dn) {
            float4* const planes[2] = {I->d_dn_plane[0].ptr, I->d_dn_plane[1].ptr};
            const float4* x0 = nullptr;
            if (dnt) { // behind the filter stage of the image before: it wrote the history this one reads, and read the one this one writes
                const uint32_t h = I->dn_image & 1u;
                if (O->dn_chain_pending) HIP_TRY(I, hipStreamWaitEvent(main, O->dn_chain, 0));
                const float v[12] = {view.pos.x, view.pos.y, view.pos.z, view.p1.x, view.p1.y, view.p1.z, view.right.x, view.right.y, view.right.z, view.up.x, view.up.y, view.up.z};
                std::memcpy(O->dn_view[h], v, sizeof(v));
                DnMotionLaunch ml{};
                DnDeformLaunch dl{};
                if (dnm) { // the snapshot of the TLAS this frame traced with, and the records against the previous image's
                    Instance* const T = tlas_of(I);
                    const uint32_t n_inst = (uint32_t)T->n_instances;
                    HIP_TRY(I, O->d_dn_snapshot[h].ensure(std::max<size_t>(n_inst, 1) * kDnInstanceBytes));
                    HIP_TRY(I, O->d_dn_motion.ensure(std::max<size_t>(n_inst, 1) * kDnMotionBytes));
                    DnDeformMotion dm{};
                    if (dnd) { // the skinned copies of the scene this frame traced (they change only with a synchronize(), which drains the frames in flight)
                        std::vector<uint4> copies;
                        uint32_t total = 0;
                        for (const auto& kv : O->derived) {
                            const MeshRecord& r = O->mesh_records[kv.second.record];
                            copies.push_back(make_uint4(r.tri_base, r.tri_count, total, kv.second.record));
                            total += r.tri_count;
                        }
                        if (copies.size() != O->dn_copies.size() || (!copies.empty() && std::memcmp(copies.data(), O->dn_copies.data(), copies.size() * sizeof(uint4)) != 0)) {
                            HIP_TRY(I, O->d_dn_copies.ensure(copies.size()));
                            O->dn_copies = copies; // (the copy reads the owner's vector, which stays as it is until the table changes again)
                            if (!copies.empty()) HIP_TRY(I, hipMemcpyAsync(O->d_dn_copies.ptr, O->dn_copies.data(), copies.size() * sizeof(uint4), hipMemcpyHostToDevice, main));
                        }
                        HIP_TRY(I, O->d_dn_refs[h].ensure(std::max<size_t>(n_inst, 1)));
                        if (total) HIP_TRY(I, O->d_dn_pose[h].ensure(4 * (size_t)total));
                        O->dn_pose_tris[h] = total;
                        dm.copies = O->d_dn_copies.ptr;
                        dm.n_copies = (uint32_t)copies.size();
                        dm.prev_refs = I->dn_image ? O->d_dn_refs[h ^ 1u].ptr : nullptr;
                        dm.cur_refs = O->d_dn_refs[h].ptr;
                        launch_dn_pose(main, sc[0].triangles, O->d_dn_copies.ptr, dm.n_copies, total, O->d_dn_pose[h].ptr);
                        dl.tris = I->d_dn_tris.ptr;
                        dl.refs = O->d_dn_refs[h].ptr;
                        dl.prev_refs = dm.prev_refs;
                        dl.prev_pose = I->dn_image ? O->d_dn_pose[h ^ 1u].ptr : nullptr;
                    }
                    launch_dn_motion(main, T->d_forward, T->d_xforms.ptr, T->d_normals.ptr, n_inst, I->dn_image ? O->d_dn_snapshot[h ^ 1u].ptr : nullptr,
                                     O->dn_snap_count[h ^ 1u], O->d_dn_snapshot[h].ptr, O->d_dn_motion.ptr, dnd ? &dm : nullptr);
                    O->dn_snap_count[h] = O->dn_motion_count = n_inst;
                    ml.ids = I->d_dn_ids.ptr;
                    ml.prev_ids = I->dn_image ? O->d_dn_history_ids[h ^ 1u].ptr : nullptr;
                    ml.cur_ids = O->d_dn_history_ids[h].ptr;
                    ml.records = O->d_dn_motion.ptr;
                    ml.n_records = n_inst;
                }
                launch_dn_temporal(main, cam[0], I->d_acc_slab.ptr, I->cap_v, I->d_dn_guide.ptr, I->dn_image ? O->d_dn_history[h ^ 1u].ptr : nullptr, O->d_dn_history[h].ptr,
                                   O->dn_view[h ^ 1u], I->sample_count, O->denoise_temporal, dnm ? &ml : nullptr, dnd ? &dl : nullptr);
                O->dn_latest = h;
                O->dn_deform_latest = dnd;
                x0 = O->d_dn_history[h].ptr;
            }
            launch_atrous(main, cam[0], I->d_acc_slab.ptr, I->cap_v, I->d_dn_guide.ptr, planes, I->d_frame_out.ptr, I->sample_count, I->denoise, I->denoise_colour,
                          I->denoise_form, x0);
            if (dnt) {
                HIP_TRY(I, hipEventRecord(O->dn_chain, main));
                O->dn_chain_pending = true;
            }
        }
        else if (mode == RFW_HIP_RENDER_FILTERED_SSAO) launch_ao_filter(main, cam[0], I->d_acc_slab.ptr, I->cap_v, I->d_ao_guide.ptr, I->d_frame_out.ptr, I->sample_count);
        else launch_assemble(main, cam[0], I->d_acc_slab.ptr, false, false, I->cap_v, I->d_frame_out.ptr, I->sample_count, mode != RFW_HIP_RENDER_DEFAULT);
        I->acc_source = I->d_acc_slab.ptr; I->acc_source_rgb = false; I->acc_source_batch = frames_out;
        if (disp) { // the display transform, in place at the render size: the accumulator and the denoiser's history never see it
            const uint64_t px = (uint64_t)I->width * I->height;
            if (O->display.automatic) {
                if (!I->d_disp_hist.ptr) { // the 256 words this slot's frames count into: zeroed once, every resolve leaves them zero
                    HIP_TRY(I, I->d_disp_hist.ensure(kDisplayHistWords));
                    HIP_TRY(I, hipMemsetAsync(I->d_disp_hist.ptr, 0, kDisplayHistWords * sizeof(uint32_t), main));
                }
                HIP_TRY(I, O->d_disp_state.ensure(kDisplayStateWords + 256u));
                if (!O->disp_chain) HIP_TRY(I, hipEventCreateWithFlags(&O->disp_chain, hipEventDisableTiming));
                float* const frame_e = reinterpret_cast<float*>(I->d_disp_hist.ptr + 256);
                launch_display_hist(main, I->d_frame_out.ptr, px, I->d_disp_hist.ptr);
                // behind the resolve of the frame before, in call order: it wrote the record this one reads
                if (O->disp_chain_pending) HIP_TRY(I, hipStreamWaitEvent(main, O->disp_chain, 0));
                launch_display_resolve(main, O->display, O->disp_have_state, I->d_disp_hist.ptr, O->d_disp_state.ptr, frame_e, O->d_disp_state.ptr + kDisplayStateWords);
                HIP_TRY(I, hipEventRecord(O->disp_chain, main));
                O->disp_chain_pending = true;
                O->disp_have_state = true;
                O->disp_latest = 2u;
                launch_display_apply(main, O->display, frame_e, I->d_frame_out.ptr, px);
            } else {
                launch_display_apply(main, O->display, nullptr, I->d_frame_out.ptr, px);
                O->disp_latest = 1u;
                O->disp_manual = O->display.exposure;
            }
        }
        if (scaled(I)) // the render scale: every frame this call leaves behind -> the window size; from here on the window frame is THE frame
            launch_resample(main, I->d_frame_out.ptr, I->width, I->height, I->d_frame_win.ptr, I->window_w, I->window_h, O->scale_filter, frames_out);
        if (ov) { // the 2D layer, in place over the frame the finaliser just wrote (behind the history's event: the history never sees it)
            const uint32_t n = ov->n_prims;
            OvFrame f;
            std::memcpy(f.view, O->view_2d->m, sizeof(f.view));
            f.width = I->window_w; f.height = I->window_h; // (the 2D layer is drawn at the window's resolution whatever the render scale)
            f.n_prims = n; f.n_draws = ov->n_draws; f.n_textures = O->n_textures;
            f.bins_x = (I->window_w + kOvBin - 1u) / kOvBin; f.bins_y = (I->window_h + kOvBin - 1u) / kOvBin;
            f.chunks = (n + 63u) / 64u;
            const size_t n_words = (size_t)f.bins_x * f.bins_y * f.chunks;
            HIP_TRY(I, I->d_ov_prims.ensure(n));
            HIP_TRY(I, I->d_ov_tap.ensure(n));
            HIP_TRY(I, I->d_ov_words.ensure(n_words));
            launch_overlay(main, f, ov->vertices.ptr, ov->draws.ptr, I->d_ov_prims.ptr, I->d_ov_tap.ptr, I->d_ov_words.ptr, O->d_tex_data.ptr, O->d_tex_desc.ptr,
                           window_frame(I));
            I->ov_frame_prims = n;
            I->ov_frame_words = (uint32_t)n_words;
        }
    }
    if (I->external_slab) // this rank's contribution to the all-gather, [frame][sub-shard][slot] in the instance's gather format
        pack_slabs(I, main, I->external_slab, frames_out);
    if (tm) (void)hipEventRecord(I->events[kEvBlit + 1], main);
    if (tm) (void)hipEventRecord(I->events[EV_FRAME1], main);
    HIP_TRY(I, hipGetLastError());
    const uint32_t passes = mode == RFW_HIP_RENDER_DEFAULT ? bounces : 1u; // (modes 1-6: one "bounce", its shadow stage = the AO rounds)
    I->last_bounces = passes;
    I->ring_bounces[slot] = tm ? passes : 0;
    I->ring_nee[slot] = mode == RFW_HIP_RENDER_DEFAULT ? nee : ao;
    I->ao_rounds = ao_rounds;
    I->frame_index++;
    if (I->frame_index - I->drained_index > kTimingRing) I->drained_index = I->frame_index - kTimingRing;
    I->frame_recorded = tm;
    I->last_count_flag = count;
    if (I->frame_done) HIP_TRY(I, hipEventRecord(I->frame_done, main));
    return RFW_HIP_OK;
}

} // namespace rfwapi

extern "C" {

uint32_t rfw_hip_abi_version(void) { return RFW_HIP_ABI_VERSION; }
uint32_t rfw_hip_selftest_index_magic(uint32_t d, uint64_t n_max) { return index_magic(d, n_max); }


void* rfw_hip_create(uint32_t width, uint32_t height, double scale, const rfw_hip_options* o)
{
    read_env_switches(); // (the one place the library asks the environment: env_switches.h)
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        g_create_error = std::string("no HIP device available (") + (e == hipSuccess ? "0 devices" : hipGetErrorString(e)) +
                         "); this backend has no CPU fallback";
        return nullptr;
    }
    if (width == 0 || height == 0) {
        g_create_error = "width and height must be non-zero";
        return nullptr;
    }
    uint32_t rw = 0, rh = 0;
    if (!render_size_of(width, height, scale, rw, rh)) {
        g_create_error = "scale must be finite, 0 < scale <= 4, and the render size (width x scale, height x scale) at most 16384 per axis";
        return nullptr;
    }
    if ((rw != width || rh != height) && o && o->world > 1) {
        g_create_error = "a render scale that changes the frame's size is not available with world > 1 (a scaled frame is not exchanged)";
        return nullptr;
    }
    Instance* I = new Instance();
    I->window_w = width;
    I->window_h = height;
    I->width = rw;
    I->height = rh;
    int dev = -1;
    uint32_t n_slots = 1;
    if (o) {
        dev = o->device;
        if (o->max_path_length) I->max_path_length = std::min<uint32_t>(o->max_path_length, kMaxBounces);
        if (o->clamp_value > 0.0f) I->clamp_value = o->clamp_value;
        I->world = std::max<uint32_t>(o->world, 1);
        I->rank = o->rank;
        if (o->tile_size) I->tile_size = o->tile_size;
        if (o->builder) I->builder = o->builder;
        I->flags = o->flags & 15u; // the public RFW_HIP_FLAG_* bits; the others are internal (set_option)
        if (o->streams) I->substreams = std::min<uint32_t>(o->streams, kMaxSub);
        if (o->struct_size >= offsetof(rfw_hip_options, frames_in_flight) + sizeof(uint32_t)) n_slots = std::min<uint32_t>(std::max<uint32_t>(o->frames_in_flight, 1u), 24u);
        if (o->struct_size >= offsetof(rfw_hip_options, max_batch) + sizeof(uint32_t)) I->max_batch = std::min<uint32_t>(std::max<uint32_t>(o->max_batch, 1u), (uint32_t)kMaxBatch);
    }
    {
        const EnvSwitches& env = env_switches();
        if (env.has_spatial_splits) I->split_tau = env.spatial_splits; // A/B runs: the default of option "spatial_splits"
        const int pt = env.packet_trace >= 0 ? env.packet_trace : kDefaultPacketTrace; // A/B runs: the default of option "packet_trace"
        I->packet_auto = env.packet_trace < 0;
        if (pt & 1) I->flags |= kFlagPacketPrimary;
        if (pt & 2) I->flags |= kFlagPacketShadow;
        if (pt & 4) I->flags |= kFlagPacketShadowFar;
    }
    if (I->max_batch > 1 && I->substreams > 1) {
        g_create_error = "max_batch > 1 needs streams <= 1 (a batch already fills the device with one launch per stage)";
        delete I;
        return nullptr;
    }
    if (I->rank >= I->world || (I->tile_size % 8) != 0) {
        g_create_error = "invalid shard options (rank >= world, or tile_size not a multiple of 8)";
        delete I;
        return nullptr;
    }
    // AUTO: BLAS by binned SAH on the host cores (built once per mesh change, best traversal quality), TLAS by LBVH on the device
    // (rebuilt every synchronize()).  HOST_SAH / DEVICE_LBVH force one builder for both levels.
    // AUTO: meshes by binned SAH on the device (the host builder's tree quality at ~14x its speed), TLAS and skinned copies by LBVH
    // (no host round trip, so they can be rebuilt every frame without draining the stream)
    I->blas_on_device = I->builder != RFW_HIP_BUILDER_HOST_SAH;
    I->blas_sah_on_device = I->builder == RFW_HIP_BUILDER_DEVICE_SAH || I->builder == RFW_HIP_BUILDER_AUTO;
    I->tlas_on_device = I->builder != RFW_HIP_BUILDER_HOST_SAH;
    if (dev < 0) (void)hipGetDevice(&dev);
    I->device = dev;
    I->build_threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    auto bail = [&](const char* what, hipError_t err) -> void* {
        g_create_error = std::string(what) + ": " + hipGetErrorString(err);
        delete I;
        return nullptr;
    };
    if ((e = hipSetDevice(dev)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&I->own_stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    I->stream = I->own_stream;
    I->ring.assign((size_t)kTimingRing * I->substreams * kNumEvents, nullptr);
    for (auto& ev : I->ring)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return bail("hipEventCreate", e);
    I->events = I->ring.data();
    if ((e = hipEventCreateWithFlags(&I->ev_fork, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    // HIP maps streams to a handful of hardware queues in creation order and two streams sharing a queue serialise, so no
    // stream is created that is not used: sub-shard streams only when the frame is actually split
    for (uint32_t k = 0; k < I->substreams && I->substreams > 1; k++) {
        if ((e = hipStreamCreateWithFlags(&I->sub[k], hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
        if ((e = hipEventCreateWithFlags(&I->ev_join[k], hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    }
    for (int k = 0; k < Instance::kStages; k++)
        if ((e = hipEventCreateWithFlags(&I->stage_event[k], hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipHostMalloc((void**)&I->overflow_host, 64, hipHostMallocMapped)) != hipSuccess) return bail("hipHostMalloc (overflow flag)", e);
    std::memset(I->overflow_host, 0, 64); // word 0: traversal stack overflow, word 1: p2p timeout; hipHostMalloc does not zero, and a block may be recycled
    if ((e = hipHostGetDevicePointer((void**)&I->overflow_dev, I->overflow_host, 0)) != hipSuccess) return bail("hipHostGetDevicePointer", e);
    if (alloc_paths(I) != RFW_HIP_OK) {
        g_create_error = I->err;
        delete I;
        return nullptr;
    }
    (void)hipStreamSynchronize(I->stream);
    if (n_slots > 1) {
        if ((e = hipEventCreateWithFlags(&I->frame_done, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&I->scene_ready, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
        rfw_hip_options so;
        std::memset(&so, 0, sizeof(so));
        if (o) std::memcpy(&so, o, std::min<size_t>(o->struct_size ? o->struct_size : sizeof(so), sizeof(so)));
        so.struct_size = sizeof(so);
        so.device = I->device;
        so.frames_in_flight = 1;
        so.max_batch = I->max_batch;
        for (uint32_t k = 1; k < n_slots; k++) {
            Instance* c = static_cast<Instance*>(rfw_hip_create(width, height, scale, &so));
            if (!c) { // g_create_error is set
                for (Instance* d : I->slots) rfw_hip_destroy(d);
                I->slots.clear();
                rfw_hip_destroy(I);
                return nullptr;
            }
            c->scene = I;
            c->slot_index = k;
            if (hipEventCreateWithFlags(&c->frame_done, hipEventDisableTiming) != hipSuccess) {
                g_create_error = "hipEventCreate (frame slot)";
                rfw_hip_destroy(c);
                for (Instance* d : I->slots) rfw_hip_destroy(d);
                I->slots.clear();
                rfw_hip_destroy(I);
                return nullptr;
            }
            I->slots.push_back(c);
        }
    }
    return I;
}

void rfw_hip_destroy(void* inst)
{
    if (!inst) return;
    Instance* I = static_cast<Instance*>(inst);
    for (Instance* c : I->slots) rfw_hip_destroy(c); // frame slots first: they read this instance's scene
    I->slots.clear();
    {
        std::lock_guard<std::mutex> g(I->mu);
        (void)hipSetDevice(I->device);
        (void)hipDeviceSynchronize();
        if (I->scene_ready) (void)hipEventDestroy(I->scene_ready);
        if (I->frame_done) (void)hipEventDestroy(I->frame_done);
        if (I->download_done) (void)hipEventDestroy(I->download_done);
        I->d_blas_nodes.release(); I->d_tlas_nodes.release(); I->d_blas_wide.release(); I->d_tlas_wide.release(); I->d_blas_oct.release(); I->d_blas_oct_abs.release(); I->d_tlas_oct.release(); I->d_blas_raw.release(); I->d_tlas_raw.release(); I->d_packets.release(); I->d_triangles.release();
        I->d_mesh_records.release(); I->d_matrices.release(); I->d_mesh_of_instance.release(); I->d_tlas_prims.release();
        I->d_xforms.release(); I->d_normals.release();
        for (auto& tb : I->tables) { tb.materials.release(); tb.area.release(); tb.point.release(); tb.spot.release(); tb.dir.release(); }
        if (I->tables_ready) (void)hipEventDestroy(I->tables_ready);
        if (I->upload_stream) (void)hipStreamDestroy(I->upload_stream);
        I->d_spill.release(); I->d_counters.release(); I->d_tex_data.release(); I->d_tex_desc.release(); I->d_blue_noise.release();
        I->d_valid_gids.release(); I->d_stage_dev.release(); I->d_tlas_order.release(); I->d_node_count.release(); I->d_inst_boxes.release(); I->d_mesh_local.release();
        I->d_tri_boxes.release(); I->d_lbvh_ws.release(); I->d_blas_order.release();
        I->d_q_o.release(); I->d_q_d.release(); I->d_q_t.release(); I->d_q_h.release(); I->d_q_depth.release(); I->d_q_r.release();
        if (I->comm) { (void)g_rccl.comm_destroy(I->comm); I->comm = nullptr; }
        if (I->loop) loop_leave(I);
        if (I->loop_sent) { (void)hipEventDestroy(I->loop_sent); I->loop_sent = nullptr; }
        if (I->comm_chain) (void)hipEventDestroy(I->comm_chain);
        for (auto& ev : I->ev_build)
            if (ev) (void)hipEventDestroy(ev);
        if (I->records_stream) (void)hipStreamSynchronize(I->records_stream);
        if (I->ev_heads) (void)hipEventDestroy(I->ev_heads);
        if (I->ev_records) (void)hipEventDestroy(I->ev_records);
        if (I->records_stream) (void)hipStreamDestroy(I->records_stream);
        I->d_heads.release();
        I->meshes.clear(); // (unregisters the pinned host copies while the runtime is still up)
        for (auto& L : I->lanes) {
            if (L.s) (void)hipStreamDestroy(L.s);
            if (L.done) (void)hipEventDestroy(L.done);
            L.ws.release(); L.boxes.release();
        }
        p2p_release(I);
        I->d_send.release(); I->d_recv.release();
        for (int q = 0; q < 2; q++) { I->d_sort_keys[q].release(); I->d_sort_vals[q].release(); }
        I->d_sort_ws.release();
        if (I->overflow_host) (void)hipHostFree(I->overflow_host);
        I->pins.release();
        I->d_skin_data.release(); I->d_joints.release(); I->d_bounds_scratch.release(); I->d_sah_ws.release(); I->d_mesh_node_counts.release(); I->d_forest.release(); I->d_refit_parent.release(); I->d_refit_nint.release(); I->d_refit_arrive.release();
        for (int k = 0; k < Instance::kStages; k++) {
            if (I->stage_buf[k]) (void)hipHostFree(I->stage_buf[k]);
            if (I->stage_event[k]) (void)hipEventDestroy(I->stage_event[k]);
        }
        for (int h = 0; h < 2; h++) { I->d_ray_o[h].release(); I->d_ray_d[h].release(); I->d_thr[h].release(); I->d_hit[h].release(); }
        I->d_sh_o.release(); I->d_sh_d.release(); I->d_sh_e.release(); I->d_acc_slab.release(); I->d_frame_acc.release(); I->d_frame_out.release(); I->d_frame_win.release(); I->d_present.release();
        I->d_dn_guide.release(); I->d_dn_plane[0].release(); I->d_dn_plane[1].release();
        I->d_dn_history[0].release(); I->d_dn_history[1].release();
        I->d_dn_ids.release(); I->d_dn_motion.release();
        for (int q = 0; q < 2; q++) { I->d_dn_history_ids[q].release(); I->d_dn_snapshot[q].release(); }
        I->release_deform();
        if (I->dn_chain) (void)hipEventDestroy(I->dn_chain);
        I->d_disp_state.release(); I->d_disp_hist.release();
        if (I->disp_chain) (void)hipEventDestroy(I->disp_chain);
        release_overlay(I);
        for (auto& ev : I->ring)
            if (ev) (void)hipEventDestroy(ev);
        if (I->ev_fork) (void)hipEventDestroy(I->ev_fork);
        for (int k = 0; k < kMaxSub; k++) {
            if (I->ev_join[k]) (void)hipEventDestroy(I->ev_join[k]);
            if (I->sub[k]) (void)hipStreamDestroy(I->sub[k]);
        }
        if (I->own_stream) (void)hipStreamDestroy(I->own_stream);
    }
    delete I;
}

const char* rfw_hip_last_error(void* inst)
{
    if (!inst) return g_create_error.c_str();
    return static_cast<Instance*>(inst)->err.c_str();
}


static int render_impl(Instance* I, const rfw_camera_view_3d* views, uint32_t k, bool samples = false, uint32_t mode = RFW_HIP_RENDER_DEFAULT)
{
    if (I->slots.empty()) return do_render(I, views, k, samples, mode);
    // frames in flight: does this call add a sample to the image of the current slot, or start a new image on the next slot?
    Instance* cur = slot_ptr(I, I->cur_slot);
    const bool same_image = (k == 1 || samples) && !I->restart && cur->sample_count > 0 && cur->have_last_view &&
                            std::memcmp(&cur->last_view, views, sizeof(*views)) == 0 && cur->rendered_version == I->scene_version &&
                            cur->render_mode == mode;
    if (!same_image) {
        I->cur_slot = (I->cur_slot + 1) % (uint32_t)(I->slots.size() + 1);
        cur = slot_ptr(I, I->cur_slot);
        cur->sample_count = 0;
    }
    I->restart = false;
    cur->rendered_version = I->scene_version;
    if (cur != I) { // the owner's options apply to every slot
        cur->max_path_length = I->max_path_length; cur->clamp_value = I->clamp_value; cur->flags = I->flags; cur->timing = I->timing;
        for (int c = 0; c < 3; c++) cur->sky[c] = I->sky[c];
        cur->ao_samples = I->ao_samples; cur->ao_radius = I->ao_radius;
        cur->denoise = I->denoise; cur->denoise_colour = I->denoise_colour; cur->denoise_form = I->denoise_form;
    }
    int rc = ensure_slot_tlas(I, cur);
    if (rc == RFW_HIP_OK) rc = do_render(cur, views, k, samples, mode);
    if (rc != RFW_HIP_OK && cur != I && !cur->err.empty()) I->err = cur->err;
    return rc;
}

int rfw_hip_render(void* inst, const rfw_mat4* view_2d, const rfw_camera_view_3d* view, uint32_t mode)
{
    LOCK(inst);
    if (!view) return fail(I, RFW_HIP_E_INVALID, "render: null view");
    CHECK_OVERFLOW(I); // of an earlier frame or query (sticky until synchronize() rebuilds the trees)
    // unknown values render as DEFAULT (the wgpu backend shows its default output for them too)
    I->view_2d = view_2d; // (read by do_render, whichever slot runs the frame)
    const int rc = render_impl(I, view, 1, false, mode <= (uint32_t)RFW_HIP_RENDER_FILTERED_SSAO ? mode : (uint32_t)RFW_HIP_RENDER_DEFAULT);
    I->view_2d = nullptr;
    return rc;
}

int rfw_hip_render_batch(void* inst, const rfw_camera_view_3d* views, uint32_t count)
{
    LOCK(inst);
    if (!views || count == 0) return fail(I, RFW_HIP_E_INVALID, "render_batch: no views");
    CHECK_OVERFLOW(I);
    if (count == 1) { // a batch of one is still a NEW image
        I->sample_count = 0;
        I->restart = true;
    }
    const int rc = render_impl(I, views, count);
    if (rc == RFW_HIP_OK && count == 1) (I->slots.empty() ? I : slot_ptr(I, I->cur_slot))->after_batch = true;
    return rc;
}

int rfw_hip_render_samples(void* inst, const rfw_camera_view_3d* view, uint32_t count)
{
    LOCK(inst);
    if (!view || count == 0) return fail(I, RFW_HIP_E_INVALID, "render_samples: no view / no samples");
    CHECK_OVERFLOW(I);
    if (count > I->max_batch || count > (uint32_t)kMaxBatch) return fail(I, RFW_HIP_E_INVALID, "render_samples: more samples than options.max_batch");
    if (count == 1) return render_impl(I, view, 1);
    rfw_camera_view_3d views[kMaxBatch];
    for (uint32_t f = 0; f < count; f++) views[f] = *view;
    return render_impl(I, views, count, true);
}


int rfw_hip_resize(void* inst, uint32_t w, uint32_t h, double scale)
{
    LOCK(inst);
    if (w == 0 || h == 0) return fail(I, RFW_HIP_E_INVALID, "resize: zero size");
    uint32_t rw = 0, rh = 0;
    if (!render_size_of(w, h, scale, rw, rh))
        return fail(I, RFW_HIP_E_INVALID, "resize: scale must be finite, 0 < scale <= 4, and the render size at most 16384 per axis");
    if (rw != w || rh != h) { // a scaled frame is not exchanged (include/rfw_hip.h): nothing has been touched yet
        const Instance* O = scene_of(I);
        if (I->world > 1 || O->comm || O->loop || O->p2p.data || I->external_slab)
            return fail(I, RFW_HIP_E_STATE, "resize: a render scale that changes the frame's size is not available on an instance that exchanges its frame (world > 1, a communicator, the p2p exchange, a slab output)");
    }
    if (scene_of(I)->p2p.data && (rw != I->width || rh != I->height)) return fail(I, RFW_HIP_E_STATE, "resize: disconnect the p2p exchange first (its buffers are sized for the frame)");
    HIP_TRY(I, hipSetDevice(I->device));
    HIP_TRY(I, hipStreamSynchronize(I->stream));
    for (Instance* c : I->slots) {
        const int rc = rfw_hip_resize(c, w, h, scale);
        if (rc != RFW_HIP_OK) return fail(I, rc, c->err);
    }
    I->restart = true;
    I->window_w = w;
    I->window_h = h;
    I->width = rw;
    I->height = rh;
    I->dn_images = 0; // option "denoise_temporal": the history belongs to the old size
    // option "denoise_motion": so do the ids, the snapshots and the records (allocated again at the next frame that needs them)
    I->d_dn_ids.release(); I->d_dn_motion.release();
    for (int q = 0; q < 2; q++) { I->d_dn_history_ids[q].release(); I->d_dn_snapshot[q].release(); I->dn_snap_count[q] = 0; }
    I->dn_motion_count = 0;
    I->release_deform(); // option "denoise_deform": and the triangle plane, the pose snapshots and their tables
    I->disp_have_state = false; I->disp_latest = 0; // the display transform adapted to frames of the old size
    I->ov_frame_prims = I->ov_frame_words = 0; // the 2D layer's taps describe a frame of the old size
    // a gathered frame not de-tiled yet belongs to the old size (and d_recv may move below): forget it (each slot passes here for itself)
    I->deferred = Instance::Deferred(); I->acc_source = nullptr; I->presented_valid = false;
    const int arc = alloc_paths(I); // also restarts accumulation (gpu-rt/src/lib.rs:1809)
    if (arc == RFW_HIP_OK && (scene_of(I)->comm || scene_of(I)->loop)) { // the gather buffers follow the slab size
        const size_t n = (size_t)I->capacity * I->max_batch * 3u;
        HIP_TRY(I, I->d_send.ensure(n));
        HIP_TRY(I, I->d_recv.ensure(n * I->world));
    }
    return arc;
}


int rfw_hip_reset_accumulation(void* inst)
{
    LOCK(inst);
    I->sample_count = 0;
    I->restart = true; // with frame slots: the next render starts a new image (on the next slot)
    return RFW_HIP_OK;
}

int rfw_hip_set_option(void* inst, const char* key, double value)
{
    LOCK(inst);
    if (!key) return fail(I, RFW_HIP_E_INVALID, "set_option: null key");
    const std::string k(key);
    if (k == "max_path_length") I->max_path_length = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)value, kMaxBounces));
    else if (k == "clamp_value") I->clamp_value = (float)value;
    else if (k == "nee") I->flags = value != 0.0 ? (I->flags & ~RFW_HIP_FLAG_NO_NEE) : (I->flags | RFW_HIP_FLAG_NO_NEE);
    else if (k == "count_traversal") I->flags = value != 0.0 ? (I->flags | RFW_HIP_FLAG_COUNT_TRAVERSAL) : (I->flags & ~RFW_HIP_FLAG_COUNT_TRAVERSAL);
    else if (k == "shadow_order") { // which end any-hit traversals start from: 0 = default (directional lights far to near, positional near to far), 1 = all near to far, 2 = all far to near
        I->flags &= ~(kFlagNearFirstDirectional | kFlagFarFirstPositional);
        if ((int)value == 1) I->flags |= kFlagNearFirstDirectional;
        else if ((int)value == 2) I->flags |= kFlagFarFirstPositional;
    }
    else if (k == "packet_trace") { // which rays walk the tree as wavefront packets (traverse_packet.h): bit 0 camera rays, bit 1 the camera paths' shadow rays
        I->flags &= ~(kFlagPacketPrimary | kFlagPacketShadow | kFlagPacketShadowFar);
        I->packet_auto = false; // an explicit choice holds whatever the scene's size
        if ((int)value & 1) I->flags |= kFlagPacketPrimary;
        if ((int)value & 2) I->flags |= kFlagPacketShadow;
        if ((int)value & 4) I->flags |= kFlagPacketShadowFar; // bit 2: packets only for the buckets traced far to near (the directional lights)
        if (blas_wide_wanted(I, I->n_tris) && !I->d_blas_wide.ptr && I->n_tris) {
            // packets asked for on a scene that was built without their copies of the nodes: the next synchronize() rebuilds (until then the
            // camera rays keep going one per lane)
            for (auto& kv : I->meshes) kv.second.dirty = true;
            I->meshes_dirty = true;
            I->layout_valid = false;
        }
    }
    else if (k == "single_space") { // 1: scenes of identity instances, one per mesh, are traced as one tree in one space; 0: never
        const int v = value != 0.0 ? 1 : 0;
        if (v != I->single_space_opt) {
            I->single_space_opt = v; // off: from the next frame; on: the next synchronize() qualifies the scene and prepares it
            if (v) I->instances_dirty = true;
        }
    }
    else if (k == "shade_group") { // threads per k_shade workgroup: 0 = automatic (do_render), 256, 512
        if ((int)value != 0 && (int)value != 256 && (int)value != 512) return fail(I, RFW_HIP_E_INVALID, "set_option: shade_group is 0, 256 or 512");
        I->shade_group = (int)value;
    }
    else if (k == "tlas_fused") I->tlas_fused = std::max(0, std::min(2, (int)value)); // 0: always the launch chain (lbvh_build); 1: always the one-workgroup build (up to 16 384 instances); 2: that where frames overlap (frame slots)
    else if (k == "sample_count") I->sample_count = (uint32_t)value;
    else if (k == "ao_samples" || k == "ao_radius") { // render modes 5, 6: a new image
        if (k == "ao_samples") {
            if (!(value >= 1.0 && value <= (double)kAoMaxSamples)) return fail(I, RFW_HIP_E_INVALID, "set_option: ao_samples is 1 ... 8");
            I->ao_samples = (uint32_t)value;
        } else {
            if (!(value >= 0.0) || !std::isfinite(value)) return fail(I, RFW_HIP_E_INVALID, "set_option: ao_radius is >= 0 (0 = automatic)");
            I->ao_radius = (float)value;
        }
        I->sample_count = 0;
        I->restart = true;
    }
    else if (k == "denoise" || k == "denoise_colour") { // the filter of the path-traced frame (denoise.inc): a changed value starts a new image
        if (k == "denoise") {
            if (!(value >= 0.0 && value <= (double)kDenoiseMaxPasses) || value != std::floor(value)) return fail(I, RFW_HIP_E_INVALID, "set_option: denoise is 0 (off) or 1 ... 5 passes");
            if ((uint32_t)value == I->denoise) return RFW_HIP_OK;
            I->denoise = (uint32_t)value;
        } else {
            if (!(value > 0.0) || !std::isfinite(value) || !((float)value > 0.0f) || !std::isfinite((float)value)) return fail(I, RFW_HIP_E_INVALID, "set_option: denoise_colour is > 0");
            if ((float)value == I->denoise_colour) return RFW_HIP_OK;
            I->denoise_colour = (float)value;
        }
        I->sample_count = 0;
        I->restart = true;
    }
    else if (k == "sample_offset") { // the first sample index of every image (seeds, blue noise); the sample COUNT still starts at 0.  A changed value starts a new image
        if (!(value >= 0.0 && value <= 16777216.0) || value != std::floor(value)) return fail(I, RFW_HIP_E_INVALID, "set_option: sample_offset is an integer 0 ... 2^24");
        if ((uint32_t)value == I->sample_offset) return RFW_HIP_OK;
        I->sample_offset = (uint32_t)value;
        I->sample_count = 0;
        I->restart = true;
    }
    else if (k == "denoise_temporal") { // Hmax, the longest history in samples (denoise.inc, k_dn_temporal); a changed value drops the history and starts a new image
        if (!(value >= 0.0 && value <= (double)kDenoiseMaxHistory) || value != std::floor(value)) return fail(I, RFW_HIP_E_INVALID, "set_option: denoise_temporal is 0 (off) or 1 ... 64 samples");
        if ((uint32_t)value == I->denoise_temporal) return RFW_HIP_OK;
        I->denoise_temporal = (uint32_t)value;
        I->dn_images = 0;
        I->sample_count = 0;
        I->restart = true;
    }
    else if (k == "denoise_motion") { // the temporal option follows moving instances (denoise.inc, k_dn_temporal_motion); a changed value drops the history and starts a new image
        if (value != 0.0 && value != 1.0) return fail(I, RFW_HIP_E_INVALID, "set_option: denoise_motion is 0 (off) or 1");
        if ((uint32_t)value == I->denoise_motion) return RFW_HIP_OK;
        I->denoise_motion = (uint32_t)value;
        I->dn_images = 0;
        I->sample_count = 0;
        I->restart = true;
    }
    else if (k == "denoise_deform") { // the temporal option follows skinned meshes (denoise.inc, k_dn_temporal_deform); a changed value drops the history and starts a new image
        if (value != 0.0 && value != 1.0) return fail(I, RFW_HIP_E_INVALID, "set_option: denoise_deform is 0 (off) or 1");
        if ((uint32_t)value == I->denoise_deform) return RFW_HIP_OK;
        I->denoise_deform = (uint32_t)value;
        I->release_deform(); // (hipFree waits for the frames in flight)
        for (Instance* c : I->slots) c->release_deform();
        I->dn_images = 0;
        I->sample_count = 0;
        I->restart = true;
    }
    else if (k == "material_maps") { // k_shade honours the metallic-roughness, sheen and emissive maps (shade_device.h, apply_parameter_maps); a changed value starts a new image
        if (value != 0.0 && value != 1.0) return fail(I, RFW_HIP_E_INVALID, "set_option: material_maps is 0 (off) or 1");
        if ((uint32_t)value == I->material_maps) return RFW_HIP_OK;
        I->material_maps = (uint32_t)value;
        I->sample_count = 0;
        I->restart = true;
    }
    else if (k == "denoise_form") { // measurement: which kernel form the passes take (0 = the faster one per step, 1 direct, 2 tiled); the image is the same
        if (value != 0.0 && value != 1.0 && value != 2.0) return fail(I, RFW_HIP_E_INVALID, "set_option: denoise_form is 0, 1 or 2");
        I->denoise_form = (uint32_t)value;
    }
    else if (k == "scale_filter") { // how the render-size frame becomes the window-size one (resample.inc): 0 nearest, 1 bilinear / area; from the next frame on, the image goes on
        if (value != 0.0 && value != 1.0) return fail(I, RFW_HIP_E_INVALID, "set_option: scale_filter is 0 (nearest) or 1 (bilinear / area)");
        I->scale_filter = (uint32_t)value;
    }
    else if (k == "tonemap" || k == "exposure" || k == "tonemap_white" || k == "auto_exposure" || k == "exposure_key" || k == "exposure_min" || k == "exposure_max" ||
             k == "exposure_low" || k == "exposure_high" || k == "exposure_speed") {
        // the display transform (display.inc): from the next frame on, the image goes on; any of them drops the adaptation state
        DisplayParams& d = I->display;
        const float f = (float)value;
        const bool integer = std::isfinite(value) && value == std::floor(value);
        auto within = [&](float lo, float hi) { return std::isfinite(value) && value >= (double)lo && value <= (double)hi && f >= lo && f <= hi; };
        if (k == "tonemap") {
            if (!integer || value < 0.0 || value > 3.0) return fail(I, RFW_HIP_E_INVALID, "set_option: tonemap is 0 (off), 1 (exposure only), 2 (extended Reinhard) or 3 (ACES fit)");
            d.curve = (uint32_t)value;
        } else if (k == "exposure") {
            if (!within(0x1p-20f, 0x1p20f)) return fail(I, RFW_HIP_E_INVALID, "set_option: exposure is 2^-20 ... 2^20");
            d.exposure = f;
        } else if (k == "tonemap_white") {
            if (!std::isfinite(value) || !(value > 0.0) || !(f > 0.0f) || !std::isfinite(f)) return fail(I, RFW_HIP_E_INVALID, "set_option: tonemap_white is finite and > 0");
            d.white = f;
        } else if (k == "auto_exposure") {
            if (value != 0.0 && value != 1.0) return fail(I, RFW_HIP_E_INVALID, "set_option: auto_exposure is 0 or 1");
            d.automatic = (uint32_t)value;
        } else if (k == "exposure_key") {
            if (!within(0x1p-10f, 0x1p10f)) return fail(I, RFW_HIP_E_INVALID, "set_option: exposure_key is 2^-10 ... 2^10");
            d.key = f;
        } else if (k == "exposure_min") {
            if (!within(0x1p-20f, d.exposure_max)) return fail(I, RFW_HIP_E_INVALID, "set_option: exposure_min is 2^-20 ... exposure_max");
            d.exposure_min = f;
        } else if (k == "exposure_max") {
            if (!within(d.exposure_min, 0x1p20f)) return fail(I, RFW_HIP_E_INVALID, "set_option: exposure_max is exposure_min ... 2^20");
            d.exposure_max = f;
        } else if (k == "exposure_low") {
            if (!integer || value < 0.0 || !(value < (double)d.high)) return fail(I, RFW_HIP_E_INVALID, "set_option: exposure_low is an integer percentage, 0 <= low < exposure_high");
            d.low = (uint32_t)value;
        } else if (k == "exposure_high") {
            if (!integer || !(value > (double)d.low) || value > 100.0) return fail(I, RFW_HIP_E_INVALID, "set_option: exposure_high is an integer percentage, exposure_low < high <= 100");
            d.high = (uint32_t)value;
        } else {
            if (!std::isfinite(value) || !(value > 0.0) || value > 1.0 || !(f > 0.0f)) return fail(I, RFW_HIP_E_INVALID, "set_option: exposure_speed is in (0, 1]");
            d.speed = f;
        }
        I->disp_have_state = false;
        I->disp_latest = 0;
    }
    else if (k == "gather_format") { // 0 f32 accumulator RGB, 1 f16 finished frame, 2 presented BGRA8 (sharded frames only)
        if (value < 0 || value > 2) return fail(I, RFW_HIP_E_INVALID, "set_option: gather_format is 0, 1 or 2");
        I->gather_format = (uint32_t)value;
        for (uint32_t q = 0; q <= I->slots.size(); q++) { // every slot: a frame gathered in the old format must not be de-tiled in the new one
            Instance* c = slot_ptr(I, q);
            c->deferred = Instance::Deferred(); c->acc_source = nullptr; c->presented_valid = false;
        }
    }
    else if (k == "present_rank") I->present_rank = (int)value;
    else if (k == "timing") I->timing = value != 0.0;
    else if (k == "sort_extension_rays") I->sort_extension_rays = std::max(0, std::min(2, (int)value));
    else if (k == "texture_array") { I->texture_array = value != 0.0; I->tex_offsets.clear(); } // applies to textures set from now on (all of them: no partial update across the switch)
    else if (k == "spill_rows") { // tests: exercise the overflow path
        I->spill_rows = std::min<uint32_t>((uint32_t)std::max(0.0, value), (uint32_t)kStackSpill);
        clear_overflow(I); // an overflow seen with another stack size says nothing about this one
    }
    else if (k == "sky_r") I->sky[0] = (float)value;
    else if (k == "sky_g") I->sky[1] = (float)value;
    else if (k == "sky_b") I->sky[2] = (float)value;
    else if (k == "sah_max_leaf") I->sah_max_leaf = std::max(1, std::min((int)value, kMaxLeafTris));
    else if (k == "sah_trav_cost") I->sah_trav_cost = (float)value;
    else if (k == "spatial_splits") I->split_tau = (float)std::max(0.0, value); // meshes handed over from now on: a part of a triangle is cut while its box wastes more than this x the mesh box's area; 0 = off
    else if (k == "stream_run") {
        const uint32_t r = (uint32_t)value;
        if (r != 0 && (r > 64 || (r & (r - 1)) != 0)) return fail(I, RFW_HIP_E_INVALID, "set_option: stream_run must be 0 or a power of two up to 64");
        I->stream_run = r;
        I->stream_auto = false;
    } else if (k == "stream_auto") { I->stream_auto = value != 0.0;
    } else if (k == "stream_leaf_gate") I->stream_leaf_gate = (uint32_t)std::max(1.0, std::min(64.0, value));
    else if (k == "stream_refill") I->stream_refill = (uint32_t)std::max(1.0, std::min(64.0, value));
    else if (k == "p2p_timeout_ms") I->p2p.timeout_ticks = (uint64_t)std::max(1.0, value) * 100000ull;
    else if (k == "build_threads") I->build_threads = std::max(1, (int)value);
    else return fail(I, RFW_HIP_E_INVALID, "set_option: unknown key " + k);
    return RFW_HIP_OK;
}

// de-tiles the linear accumulator of the latest frame(s) into d_frame_acc, on the instance's stream (zeros before the first frame)
static int materialize_accumulator(Instance* I)
{
    if (scene_of(I)->gather_format != 0 && gathers_tiles(I))
        return fail(I, RFW_HIP_E_STATE, "read_accumulator: with gather_format 1 / 2 only the finished frame travels; the accumulators stay on the ranks that own the tiles");
    { const int rc = ensure_assembled(I); if (rc != RFW_HIP_OK) return rc; }
    const size_t px = (size_t)I->width * I->height * I->max_batch;
    HIP_TRY(I, I->d_frame_acc.ensure(px));
    if (!I->acc_source) {
        HIP_TRY(I, hipMemsetAsync(I->d_frame_acc.ptr, 0, px * sizeof(float4), I->stream));
        return RFW_HIP_OK;
    }
    CameraParams cam = camera_params(I, I->last_view);
    cam.batch = I->acc_source_batch;
    launch_assemble(I->stream, cam, I->acc_source, I->acc_source_rgb, true, I->cap_v, I->d_frame_acc.ptr, 1u);
    HIP_TRY(I, hipGetLastError());
    return RFW_HIP_OK;
}
static int read_frame_impl(void* inst, uint32_t frame, bool accumulator, float* rgba, uint64_t n);
int rfw_hip_read_framebuffer_at(void* inst, uint32_t frame, float* rgba, uint64_t n) { return read_frame_impl(inst, frame, false, rgba, n); }
int rfw_hip_read_accumulator_at(void* inst, uint32_t frame, float* rgba, uint64_t n) { return read_frame_impl(inst, frame, true, rgba, n); }
static int read_frame_impl(void* inst, uint32_t frame, bool accumulator, float* rgba, uint64_t n)
{
    LOCK(inst);
    // the accumulator lives at the render size, the finished frame at the window size
    const uint64_t fpx = accumulator ? (uint64_t)I->width * I->height : (uint64_t)I->window_w * I->window_h;
    if (!rgba || n != fpx * 4) return fail(I, RFW_HIP_E_INVALID, "read_*_at: size mismatch");
    if (frame >= I->max_batch) return fail(I, RFW_HIP_E_INVALID, "read_*_at: frame index beyond options.max_batch");
    if (!I->slots.empty() && I->cur_slot != 0) { // frames in flight: the latest batch lives in a slot
        Instance* c = slot_ptr(I, I->cur_slot);
        const int rc = read_frame_impl(c, frame, accumulator, rgba, n);
        if (rc != RFW_HIP_OK) I->err = c->err;
        return rc;
    }
    HIP_TRY(I, hipSetDevice(I->device));
    if (accumulator) {
        const int rc = materialize_accumulator(I);
        if (rc != RFW_HIP_OK) return rc;
    } else {
        if (scene_of(I)->gather_format == 2 && gathers_tiles(I))
            return fail(I, RFW_HIP_E_STATE, "read_framebuffer: gather_format 2 leaves the PRESENTED frame only: rfw_hip_download_frame(what = 2)");
        const int rc = ensure_assembled(I);
        if (rc != RFW_HIP_OK) return rc;
    }
    const float4* src = (accumulator ? I->d_frame_acc.ptr : window_frame(I)) + (size_t)frame * fpx;
    HIP_TRY(I, hipMemcpyAsync(rgba, src, n * sizeof(float), hipMemcpyDeviceToHost, I->stream));
    HIP_TRY(I, hipStreamSynchronize(I->stream));
    CHECK_OVERFLOW(I);
    return RFW_HIP_OK;
}

// step k = the smallest linear value whose sRGB encoding rounds to byte k + 1: srgb_to_linear((k + 0.5) / 255), IEC 61966-2-1
void rfw_hip_srgb_steps(float* out255)
{
    if (out255) std::memcpy(out255, srgb_steps(), 255 * sizeof(float));
}
// Pinned host memory for rfw_hip_download_frame (a pageable destination would make the copy synchronous and staged)
void* rfw_hip_host_alloc(uint64_t bytes)
{
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void rfw_hip_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}
// Queue the copy of the latest frame (what = 0: finalised frame, 1: accumulator; batch frame `frame`) to host memory behind the
// kernels that produce it, on that frame's stream, and return: with frames in flight the copy of frame k runs on the DMA engines
// while the slots of frames k+1... trace.  The bytes are valid after rfw_hip_wait_downloads.
int rfw_hip_download_frame(void* inst, uint32_t what, uint32_t frame, float* host_rgba, uint64_t n)
{
    LOCK(inst);
    const uint64_t px = what == 1 ? (uint64_t)I->width * I->height : (uint64_t)I->window_w * I->window_h; // accumulator: render size; finished frame: window
    if (!host_rgba || n != (what == 2 ? px : px * 4)) return fail(I, RFW_HIP_E_INVALID, "download_frame: size mismatch");
    if (what > 2 || frame >= I->max_batch) return fail(I, RFW_HIP_E_INVALID, "download_frame: bad selector");
    Instance* c = I->slots.empty() ? I : slot_ptr(I, I->cur_slot);
    HIP_TRY(I, hipSetDevice(I->device));
    if (!c->download_done) HIP_TRY(I, hipEventCreateWithFlags(&c->download_done, hipEventDisableTiming));
    if (what == 1) {
        const int rc = materialize_accumulator(c);
        if (rc != RFW_HIP_OK) return fail(I, rc, c->err);
    } else {
        const int rc = ensure_assembled(c);
        if (rc != RFW_HIP_OK) return fail(I, rc, c->err);
    }
    const bool sharded_presented = scene_of(c)->gather_format == 2 && gathers_tiles(c);
    if (sharded_presented) { // the gathered frame IS the presented frame: de-tiled into d_present already, nothing to encode
        if (what != 2) return fail(I, RFW_HIP_E_STATE, "download_frame: gather_format 2 leaves the PRESENTED frame only (what = 2)");
        if (!c->presented_valid) return fail(I, RFW_HIP_E_STATE, "download_frame: no gathered frame yet");
        HIP_TRY(I, hipMemcpyAsync(host_rgba, c->d_present.ptr + (size_t)frame * px, px * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(I, hipEventRecord(c->download_done, c->stream));
        c->download_dst.push_back(host_rgba);
        return RFW_HIP_OK;
    }
    const float4* src = (what == 1 ? c->d_frame_acc.ptr : window_frame(c)) + (size_t)frame * px;
    // Presented frame into a pinned destination (rfw_hip_host_alloc, or registered by the caller): the encoding kernel stores straight
    // into host memory over the link, no copy command (measured: 0.731 ms per frame against 0.762 with encode + copy, 8 frames in flight).
    // Float frames, and pageable destinations, go through the runtime's copy.
    void* mapped = nullptr;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, host_rgba) == hipSuccess && attr.type == hipMemoryTypeHost) mapped = attr.devicePointer;
    else (void)hipGetLastError();
    if (what == 2) { // the swap-chain image: encode on the device, a quarter of the bytes travel
        uint32_t* out = (uint32_t*)mapped;
        if (!out) {
            HIP_TRY(I, c->d_present.ensure(px));
            out = c->d_present.ptr;
        }
        launch_present(c->stream, src, out, px, srgb_steps(), mapped != nullptr);
        HIP_TRY(I, hipGetLastError());
        if (!mapped) HIP_TRY(I, hipMemcpyAsync(host_rgba, c->d_present.ptr, px * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    } else { // 33 MB per 1080p frame: the DMA engine moves it at ~40 GB/s; stores from a kernel reach ~28 GB/s (measured)
        HIP_TRY(I, hipMemcpyAsync(host_rgba, src, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(I, hipEventRecord(c->download_done, c->stream));
    c->download_dst.push_back(host_rgba);
    return RFW_HIP_OK;
}
// host_ptr == NULL: every copy queued so far; else the copy into host_ptr (and, being on the same stream, those queued before it on its slot)
int rfw_hip_wait_download(void* inst, const void* host_ptr)
{
    LOCK(inst);
    HIP_TRY(I, hipSetDevice(I->device));
    for (size_t k = 0; k <= I->slots.size(); k++) {
        Instance* c = slot_ptr(I, (uint32_t)k);
        if (c->download_dst.empty()) continue;
        if (host_ptr && std::find(c->download_dst.begin(), c->download_dst.end(), host_ptr) == c->download_dst.end()) continue;
        HIP_TRY(I, hipEventSynchronize(c->download_done)); // the event is behind the LAST copy of this slot
        c->download_dst.clear();
    }
    return RFW_HIP_OK;
}
int rfw_hip_wait_downloads(void* inst) { return rfw_hip_wait_download(inst, nullptr); }

// the latest frame (frame 0 of a batch)
int rfw_hip_read_framebuffer(void* inst, float* rgba, uint64_t n) { return read_frame_impl(inst, 0, false, rgba, n); }
int rfw_hip_read_accumulator(void* inst, float* rgba, uint64_t n) { return read_frame_impl(inst, 0, true, rgba, n); }

static void add_frame_timing(Instance* I, int slot, uint32_t nb, bool nee, rfw_hip_frame_stats* out)
{
    hipEvent_t* e0 = ring_events(I, slot, 0);
    auto el = [&](hipEvent_t a, hipEvent_t b) { float ms = 0.0f; (void)hipEventElapsedTime(&ms, a, b); return ms; };
    out->ms_total += el(e0[EV_FRAME0], e0[EV_FRAME1]);
    out->ms_other += el(e0[kEvBlit], e0[kEvBlit + 1]);
    // per-kernel figures are SUMS over the sub-shard launches (which overlap in time on different streams)
    for (uint32_t s = 0; s < I->substreams; s++) {
        hipEvent_t* ev = ring_events(I, slot, s);
        for (uint32_t b = 0; b < nb; b++) {
            const float tr = el(ev[ev_index(b, 0, 0)], ev[ev_index(b, 0, 1)]);
            if (b == 0) out->ms_trace_primary += tr; else out->ms_trace_extend += tr;
            out->ms_shade += el(ev[ev_index(b, 1, 0)], ev[ev_index(b, 1, 1)]);
            if (nee) out->ms_trace_shadow += el(ev[ev_index(b, 2, 0)], ev[ev_index(b, 2, 1)]);
        }
    }
}

int rfw_hip_get_frame_stats(void* inst, rfw_hip_frame_stats* out)
{
    LOCK(inst);
    if (!out) return fail(I, RFW_HIP_E_INVALID, "get_frame_stats: null out");
    if (!I->slots.empty() && I->cur_slot != 0) { // frames in flight: the latest frame lives in a slot
        Instance* c = slot_ptr(I, I->cur_slot);
        const int rc = rfw_hip_get_frame_stats(c, out);
        if (rc != RFW_HIP_OK) I->err = c->err;
        return rc;
    }
    HIP_TRY(I, hipSetDevice(I->device));
    std::memset(out, 0, sizeof(*out));
    HIP_TRY(I, hipStreamSynchronize(I->stream));
    QueueCounters qc[kMaxSub];
    HIP_TRY(I, hipMemcpy(qc, I->d_counters.ptr + (size_t)I->counter_phase * kMaxSub, I->substreams * sizeof(QueueCounters), hipMemcpyDeviceToHost));
    CHECK_OVERFLOW(I);
    const uint32_t nb = I->last_bounces;
    out->primary_rays = nb ? I->local_pixels : 0;
    for (uint32_t s = 0; s < I->substreams; s++) {
        for (uint32_t b = 0; b + 1 < nb; b++) out->extension_rays += qc[s].ext[b];
        if (!(I->flags & RFW_HIP_FLAG_NO_NEE))
            for (uint32_t b = 0; b < nb; b++)
                for (int k = 0; k < kShadowBuckets; k++) out->shadow_rays += qc[s].shadow[b][k];
        for (int k = 0; k < 3; k++) {
            out->nodes_visited[k] += qc[s].trav[k][0];
            out->tris_tested[k] += qc[s].trav[k][1];
            out->instances_entered[k] += qc[s].trav[k][2];
            out->node_test_executions[k] += qc[s].wave_exec[k][0];
            out->tri_test_executions[k] += qc[s].wave_exec[k][1];
            out->uniform_node_test_executions[k] += qc[s].wave_uniform[k];
            out->wave_max_nodes[k] += qc[s].wave_max_nodes[k];
        }
    }
    out->sample_count = I->sample_count;
    out->bounces = nb;
    out->substreams = I->substreams;
    if (I->frame_recorded && nb) add_frame_timing(I, (int)((I->frame_index - 1) % kTimingRing), nb, !(I->flags & RFW_HIP_FLAG_NO_NEE), out);
    return RFW_HIP_OK;
}

int rfw_hip_drain_timing(void* inst, rfw_hip_frame_stats* sum, uint32_t* frames)
{
    LOCK(inst);
    if (!sum || !frames) return fail(I, RFW_HIP_E_INVALID, "drain_timing: null out");
    HIP_TRY(I, hipSetDevice(I->device));
    HIP_TRY(I, hipStreamSynchronize(I->stream));
    std::memset(sum, 0, sizeof(*sum));
    uint32_t n = 0;
    for (uint64_t f = I->drained_index; f < I->frame_index; f++) {
        const int slot = (int)(f % kTimingRing);
        const uint32_t nb = I->ring_bounces[slot];
        if (!nb) continue;
        add_frame_timing(I, slot, nb, I->ring_nee[slot], sum);
        n++;
    }
    sum->substreams = I->substreams;
    I->drained_index = I->frame_index;
    for (Instance* c : I->slots) { // frames in flight: the timings of every slot's frames
        rfw_hip_frame_stats cs;
        uint32_t cn = 0;
        const int rc = rfw_hip_drain_timing(c, &cs, &cn);
        if (rc != RFW_HIP_OK) return fail(I, rc, c->err);
        sum->ms_total += cs.ms_total; sum->ms_trace_primary += cs.ms_trace_primary; sum->ms_trace_extend += cs.ms_trace_extend;
        sum->ms_trace_shadow += cs.ms_trace_shadow; sum->ms_shade += cs.ms_shade; sum->ms_other += cs.ms_other;
        n += cn;
    }
    *frames = n;
    return RFW_HIP_OK;
}


int rfw_hip_set_stream(void* inst, void* stream)
{
    LOCK(inst);
    if (!I->slots.empty()) return fail(I, RFW_HIP_E_STATE, "set_stream: an instance with frames in flight launches on its slots' own streams");
    HIP_TRY(I, hipSetDevice(I->device));
    HIP_TRY(I, hipStreamSynchronize(I->stream));
    I->stream = stream ? (hipStream_t)stream : I->own_stream;
    return RFW_HIP_OK;
}

int rfw_hip_get_render_size(void* inst, uint32_t* width, uint32_t* height)
{
    LOCK(inst);
    if (!width || !height) return fail(I, RFW_HIP_E_INVALID, "get_render_size: null out");
    *width = I->width;
    *height = I->height;
    return RFW_HIP_OK;
}

void* rfw_hip_get_stream(void* inst)
{
    if (!inst) return nullptr;
    Instance* I = static_cast<Instance*>(inst);
    std::lock_guard<std::mutex> g(I->mu);
    return (void*)I->stream;
}

int rfw_hip_device_synchronize(void* inst)
{
    LOCK(inst);
    HIP_TRY(I, hipSetDevice(I->device));
    HIP_TRY(I, hipStreamSynchronize(I->stream));
    for (Instance* c : I->slots) HIP_TRY(I, hipStreamSynchronize(c->stream)); // every frame in flight
    return RFW_HIP_OK;
}

} // extern "C"
