// kernels.h — launch wrappers of the HIP kernels (defined in kernels.hip), callable from the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rfw_hip.h"
#include "device_types.h"

namespace rfwhip {

struct SceneDev {
    const Node4Q* tlas_nodes;
    const uint32_t* tlas_prims;
    const InstanceXform* instances;
    const InstanceNormal* instance_normals;
    const MeshRecord* meshes;         // per mesh record: where it lives, and the triangle-id offset the boundary reports
    // Single-space scenes (DESIGN.md "Single-space scenes"): the copies of blas_oct with ABSOLUTE child references (PacketNode::pad of blas_wide
    // holds the same references), or nullptr.  The trace launches take their single-space twins when ss_root != 0: the root of this frame's
    // graft in those arrays.  (Both sit where the struct had an unread pointer — the quantised mesh nodes, which no kernel reads — and four
    // bytes of padding: the kernels' argument block is laid out as it was.)
    const Node4Q* blas_oct_abs;
    // the same trees as the packet kernels read them (traverse_packet.h: a node is fetched once per wavefront through the scalar cache):
    // eight copies, one per ray octant, child boxes as floats, near / far planes picked and children sorted for the octant (PacketNode);
    // nullptr = not available
    const PacketNode* tlas_wide;
    const PacketNode* blas_wide;
    uint32_t tlas_wide_stride, blas_wide_stride; // nodes per octant copy
    // ... and as the one-ray-per-lane kernels read them (traverse.h): the same eight copies, still quantised (make_octant_node), same strides
    const Node4Q* tlas_oct;
    const Node4Q* blas_oct;
    const TriPacket* tri_packets;
    const rfw_rt_triangle* triangles; // shading attributes, global triangle id order
    const rfw_device_material* materials;
    const rfw_area_light* area_lights;
    const rfw_point_light* point_lights;
    const rfw_spot_light* spot_lights;
    const rfw_directional_light* directional_lights;
    const uint32_t* tex_data;   // all textures' texels (set_textures), then the skybox's
    const TexDesc* tex_desc;
    uint32_t n_textures;
    TexDesc skybox;             // mips == 0: no skybox image, a miss adds the constant sky colour
    uint32_t ss_root;           // != 0: a single-space frame (see blas_oct_abs)
    const uint8_t* blue_noise;  // kBlueNoiseWords table entries (each a byte), or nullptr: every sample draws from xorshift
    uint32_t* spill;
    uint32_t spill_stride;
    uint32_t spill_rows;        // <= kStackSpill
    uint32_t* overflow_flag;    // pinned host word, device-visible
    QueueCounters* counters;
    // the counter block of the NEXT frame on this instance's stream (the other half of a ring of two): k_primary clears it, so that no frame starts
    // with a clear of its own — a 512-byte fill is a dispatch like any other, and with frames in flight it queued behind the trace kernels'
    // wavefronts for up to 0.76 ms before its frame's first kernel could start (kernel timeline, round 5)
    QueueCounters* counters_next;
};

// Wavefront state, structure-of-arrays of 16-B elements (the reference's 64-B AoS PathState, structs.glsl:4-9, split):
//   ray_o  = (origin.xyz, bits(path id))        ray_d = (direction.xyz, bits(packed previous normal))
//   thr    = (throughput.rgb, postponed bsdf pdf)  hit = (inst, tri, bits(t), bary 16:16)
// two halves each (ping-pong on path_length % 2, shade.comp:77-81); shadow queue = PotentialContribution (structs.glsl:172-176)
struct PathDev {
    float4* ray_o[2];
    float4* ray_d[2];
    float4* thr[2];
    uint4* hit[2];
    float4* sh_o; // (origin.xyz, bits(pixel))
    float4* sh_d; // (direction.xyz, distance)
    float4* sh_e; // (contribution.rgb, 0)
    float4* acc;  // accumulator in slab order (this rank's tiles)
    uint32_t capacity; // local paths = local_tiles * tile_size^2
};

void launch_prepare_instances(hipStream_t s, const rfw_mat4* matrices, const uint32_t* mesh_of_instance, const MeshRecord* meshes, uint32_t n,
                              InstanceXform* xf, InstanceNormal* nm);
void launch_primary(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, bool count);
void launch_primary_batch(hipStream_t s, const CameraParams& cam, const BatchViews& views, const SceneDev& sc, const PathDev& p, bool count);
void launch_extend(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, uint32_t bounce, bool count, const uint32_t* order = nullptr);
void launch_extension_keys(hipStream_t s, const SceneDev& sc, const PathDev& p, uint32_t bounce, uint32_t* keys, uint32_t* vals);
// (cam.flags: kFlagShadeSmallGroups picks the workgroup size, kFlagMaterialMaps the twin (k_shade_maps) that reads the materials' metallic-roughness,
// sheen and emissive maps — option "material_maps"; without the flag the kernels launched are the ones that never heard of it)
void launch_shade(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, uint32_t bounce);
void launch_shadow(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, uint32_t bounce, bool count);
void launch_copy_f4(hipStream_t s, const float4* src, float4* dst, uint64_t n); // bandwidth probe
void launch_issue_probe(hipStream_t s, int mix, uint32_t cus, uint32_t trips, float* out); // issue-rate probe (mix 0, 1, 2: kernels.hip)
uint32_t issue_probe_vector_per_trip(int mix);                                                // vector instructions per trip and wavefront of that mix
// The eight per-octant copies of a node array (PacketNode for the packet kernels, Node4Q for the one-ray-per-lane kernels): copy `oct` of
// node i at [oct * stride + i] of both
struct OctantCopies {
    PacketNode* wide = nullptr;
    Node4Q* quant = nullptr;
    uint32_t stride = 0;
};
// out[i] = quantised in[i] and its octant copies at oc[first + i], i < n.  `live` (nullable): the tree's node count ON THE DEVICE — slots behind
// it are skipped (regions are sized for the worst case, one node per primitive)
void launch_quantize_nodes(hipStream_t s, const Node4* in, Node4Q* out, const OctantCopies& oc, uint32_t first, uint32_t n, const uint32_t* live = nullptr);
// behind tlas_build_fused (lbvh.h): quantised nodes + their per-octant copies (the first *live of n_nodes_max) and the instance descriptors, one launch
void launch_tlas_finish(hipStream_t s, const Node4* raw, Node4Q* out, const OctantCopies& oc, uint32_t n_nodes_max, const uint32_t* live, const rfw_mat4* matrices,
                        const uint32_t* mesh_of_instance, const MeshRecord* meshes, uint32_t n_instances, InstanceXform* xf, InstanceNormal* nm);
void launch_expand_nodes(hipStream_t s, const Node4Q* in, const OctantCopies& oc, uint32_t first, uint32_t n, const uint32_t* live = nullptr); // the copies of already quantised nodes
// the same for slots [0, n) holding SEVERAL trees: record k's tree lives at recs[k].node_base and has counts[k] nodes (both on the device)
void launch_quantize_regions(hipStream_t s, const Node4* in, Node4Q* out, const OctantCopies& oc, uint32_t n, const MeshRecord* recs, const uint32_t* counts, uint32_t n_recs);
// Single-space scenes: expand — the octant copies of ONE mesh's quantised nodes (slots node_base .. node_base + n of the arrays) with
// absolute child references into abs_oct, the references also into PacketNode::pad of `wide` (nullable); live (nullable): the tree's node
// count on the device, else all n slots hold nodes.  graft —
// the TLAS tree `raw` (its first *live of n_nodes_max nodes) as nodes root .. of both arrays, its leaves replaced by the meshes' root nodes
// (room for n_nodes_max + the instance list's length).  packet_ids — TriPacket::pad of one mesh's packets = the id of its one instance.
void launch_ss_expand(hipStream_t s, const Node4Q* in, Node4Q* abs_oct, PacketNode* wide, uint32_t stride, uint32_t n, const uint32_t* live, uint32_t node_base, uint32_t tri_base);
void launch_ss_graft(hipStream_t s, const Node4* raw, uint32_t n_nodes_max, const uint32_t* live, const uint32_t* prims, const InstanceXform* xf, uint32_t root, Node4Q* abs_oct,
                     PacketNode* wide, uint32_t stride);
void launch_ss_packet_ids(hipStream_t s, TriPacket* packets, uint32_t n, uint32_t gid);
// linear: render modes 1-6 finalise as acc / samples instead of sqrt(acc / samples) (the accumulator read is the same either way)
void launch_assemble(hipStream_t s, const CameraParams& cam, const void* gathered, bool rgb, bool accumulator, uint64_t slab_elems, float4* frame,
                     uint32_t samples, bool linear = false);
void launch_sum_batch(hipStream_t s, float4* acc_slabs, uint64_t slab_elems, uint32_t count); // slab 0 += slabs 1 .. count - 1, in order
void launch_pack_rgb(hipStream_t s, const float4* acc_slab, float* out, uint64_t n);
// the FINISHED frame of a slab for the all-gather (format 1: three halves per pixel; 2: presented B, G, R, A bytes) and its de-tiling
void launch_pack_finished(hipStream_t s, const float4* acc_slab, void* out, uint64_t n, uint32_t samples, uint32_t format, const float* steps255, bool linear = false);
// peer-to-peer exchange: flag words in uncached memory.  wait: lanes first .. first + count - 1 of ONE wavefront poll flags[lane] until it has
// reached `want` (wrap-safe), at most `limit_ticks` of the 100 MHz wall clock, then *timeout_flag = 1.  signal: *targets.p[i] = value.
struct P2PTargets { uint32_t* p[16]; };
void launch_p2p_wait(hipStream_t s, const uint32_t* flags, uint32_t first, uint32_t count, uint32_t want, uint64_t limit_ticks, uint32_t* timeout_flag);
void launch_p2p_signal(hipStream_t s, const P2PTargets& targets, uint32_t count, uint32_t value);
void launch_assemble_finished(hipStream_t s, const CameraParams& cam, const void* gathered, uint64_t slab_elems, uint32_t format, float4* frame, uint32_t* presented);
void launch_present(hipStream_t s, const float4* frame, uint32_t* bgra, uint64_t n, const float* steps255, bool narrow);
constexpr uint32_t kAoMaxSamples = kShadowBuckets; // AO rays per pixel and sample: round r goes through shadow bucket r
// render modes 1-6 (aov.inc): after the primary launch, the mode's value into the accumulator slab (1-4), or the ambient occlusion rays of
// rounds 0 .. ao_samples - 1 into shadow buckets 0 .. ao_samples - 1 and the filter guide (5, 6); `direction` = the view's (mode 4)
void launch_aov(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, uint32_t mode, uint32_t ao_samples, float ao_radius, float4* guide,
                const float direction[3]);
// mode 6 where the frame is de-tiled on this device: the edge-aware filter of acc.x / samples (slabs of slab_elems, as launch_assemble) into `frame`
void launch_ao_filter(hipStream_t s, const CameraParams& cam, const float4* acc, uint64_t slab_elems, const float4* guide, float4* frame, uint32_t samples);
// option "denoise" (denoise.inc).  Guide: after the primary launch and BEFORE launch_shade, three planes of width x height per frame pixel,
// (faced gN, t), (P, 0), (albedo, f); `pixel_mask` strips the sample index a batch of samples keeps above the pixel index of the path word.
void launch_dn_guide(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, float4* guide, uint32_t pixel_mask);
// `passes` (1 .. kDenoiseMaxPasses) a-trous passes from the accumulator slabs (as launch_assemble reads them) into `frame`, in place of
// launch_assemble; planes[2]: width x height each, used when passes > 1; x0 (or null): x_0 as a plane (rgb, w > 0 where filtered).  form: 0 = the form measured to be faster per step, 1 direct, 2 tiled.
constexpr uint32_t kDenoiseMaxPasses = 5;
constexpr float kDenoiseDefaultColour = 32.0f; // option "denoise_colour" (sigma_c, demodulated radiance): chosen by the sweep in DESIGN.md "Denoiser"
void launch_atrous(hipStream_t s, const CameraParams& cam, const float4* acc, uint64_t slab_elems, const float4* guide, float4* const planes[2], float4* frame,
                   uint32_t samples, uint32_t passes, float sigma_colour, uint32_t form, const float4* x0 = nullptr);
// option "denoise_temporal": before launch_atrous, which then takes `cur` as x0.  A history is three planes of width x height ((x.rgb, h), g0, g1);
// prev = the previous image's (null: none) and prev_view = pos, p1, right, up of the frame that wrote it; max_history = Hmax, in samples.
constexpr uint32_t kDenoiseMaxHistory = 64;
void launch_dn_temporal(hipStream_t s, const CameraParams& cam, const float4* acc, uint64_t slab_elems, const float4* guide, const float4* prev, float4* cur,
                        const float prev_view[12], uint32_t samples, uint32_t max_history, const struct DnMotionLaunch* motion = nullptr,
                        const struct DnDeformLaunch* deform = nullptr);
// option "denoise_motion" (denoise.inc, DESIGN.md "Denoiser: motion").  Ids: where launch_dn_guide is, one uint32 per frame pixel, the instance
// id of the primary hit (0xffffffff: a miss).  Motion: one thread per instance of the frame's TLAS — its entry of the snapshot `cur`
// (kDnInstanceBytes each) that travels with the history this image writes, and its record (kDnMotionBytes: rows of A, rows of B, the state's
// bits in the fourth float of B's first row) against the snapshot `prev` of n_prev instances (null: no history).  launch_dn_temporal with
// `motion` runs k_dn_temporal_motion: it reads the records and both id planes and copies the frame's ids into cur_ids.
constexpr size_t kDnInstanceBytes = 128, kDnMotionBytes = 96;
struct DnMotionLaunch {
    const uint32_t* ids;
    const uint32_t* prev_ids;
    uint32_t* cur_ids;
    const void* records;
    uint32_t n_records;
};
void launch_dn_ids(hipStream_t s, const CameraParams& cam, const PathDev& p, uint32_t* ids, uint32_t pixel_mask);
// option "denoise_deform" (denoise.inc, DESIGN.md "Denoiser: deforming meshes").  Tris: where launch_dn_ids is, one uint2 per frame pixel: the
// triangle-buffer row of the primary hit (bit 31: primary_surface negated the geometric normal) and the packed barycentrics; (0xffffffff, 0): a
// miss.  Pose: tp[0..3] of every triangle of every skinned copy into `pose` (four float4 per triangle), the copies given as a device table of
// uint4 (first row, triangles, first triangle in `pose`, mesh record index) in `pose` order.  launch_dn_motion with `deform` also writes one
// uint4 per instance id (first row, triangles, first triangle in the pose snapshot, 0; all 0: no skinned copy) into cur_refs and gives state 3
// to a skinned copy of both images; launch_dn_temporal with `deform` (and `motion`) runs k_dn_temporal_deform.
struct DnDeformMotion {
    const uint4* copies;
    uint32_t n_copies;
    const uint4* prev_refs; // null: no history
    uint4* cur_refs;
};
struct DnDeformLaunch {
    const uint2* tris;
    const uint4* refs;
    const uint4* prev_refs;
    const float4* prev_pose;
};
void launch_dn_tris(hipStream_t s, const CameraParams& cam, const SceneDev& sc, const PathDev& p, uint2* tris, uint32_t pixel_mask);
void launch_dn_pose(hipStream_t s, const rfw_rt_triangle* triangles, const uint4* copies, uint32_t n_copies, uint32_t total, float4* pose);
void launch_dn_motion(hipStream_t s, const rfw_mat4* matrices, const InstanceXform* xf, const InstanceNormal* nm, uint32_t n, const void* prev, uint32_t n_prev,
                      void* cur, void* records, const DnDeformMotion* deform = nullptr);
// The 2D layer (overlay.inc, DESIGN.md "2D layer"): the trait's 2D meshes drawn over the finalised frame, in place, behind whichever of
// launch_assemble / launch_ao_filter / launch_atrous wrote it.  A draw is one (mesh, instance) pair; draws are sorted by (mesh id, instance
// index) and the primitives of the frame are their triangles in that order (the draw position).  Three launches per frame:
//   setup   one thread per primitive: transform, snap, edge functions, record (OvPrim) and debug tap (OvTap)
//   bin     one wavefront per 64 x 64 pixels: word c of a bin = the ballot of "the box of primitive 64 c + lane touches the bin"
//   raster  one workgroup per 16 x 16 pixels, one pixel per lane: walks its bin's words in draw order and blends in registers
constexpr uint32_t kOvMaxPrims = 1u << 20; // triangles x instances of one frame
constexpr uint32_t kOvBin = 64, kOvTile = 16;
struct OvDraw {
    float m[16];           // the instance matrix, column-major
    uint32_t first_prim;   // draw position of its triangle 0
    uint32_t n_tris;
    uint32_t first_vertex; // of its mesh in the vertex array
    uint32_t mesh, instance;
    int32_t tex;           // texture of set_textures, < 0: none
    uint32_t pad[2];
};
static_assert(sizeof(OvDraw) == 96, "OvDraw");
struct OvTap { // rfw_hip_debug_read "ov_prims"
    int32_t X[3], Y[3]; // the snapped vertices (8 sub-pixel bits), in the caller's vertex order
    uint32_t mesh, instance, triangle, dropped;
    uint32_t pad[2];
};
static_assert(sizeof(OvTap) == 48, "OvTap");
struct OvPrim {
    // edge i runs from vertex i to vertex i + 1 (after the swap that makes the doubled area S positive):
    // E_i at the centre of pixel (px, py) = C[i] + 256 (A[i] px + B[i] py); covered iff every E_i >= need[i] (1, or 0 on a top or left edge)
    int64_t C[3];
    int64_t S;
    int32_t A[3], B[3];
    int32_t need[3];
    int32_t tex;            // < 0: untextured
    int32_t x0, y0, x1, y1; // pixels whose centre can be covered, clipped to the frame; x0 > x1: none (dropped, or outside)
    float uv[3][2];
    float color[3][4];
};
static_assert(sizeof(OvPrim) == 160, "OvPrim");
struct OvFrame {
    float view[16]; // CameraView2D::matrix, column-major
    uint32_t width, height;
    uint32_t n_prims, n_draws, n_textures;
    uint32_t bins_x, bins_y, chunks; // bins of kOvBin pixels; words per bin = ceil(n_prims / 64)
};
void launch_overlay(hipStream_t s, const OvFrame& f, const rfw_vertex_2d* vertices, const OvDraw* draws, OvPrim* prims, OvTap* tap, uint64_t* words,
                    const uint32_t* tex_data, const TexDesc* tex_desc, float4* frame);
// The render scale (resample.inc, DESIGN.md "Render scale"): `frames` finalised frames of rw x rh at `src` -> frames of w x h at `dst`; filter 0 =
// nearest, 1 = bilinear when enlarging / exact area average when shrinking (per axis).  Issued only where the two sizes differ.
void launch_resample(hipStream_t s, const float4* src, uint32_t rw, uint32_t rh, float4* dst, uint32_t w, uint32_t h, uint32_t filter, uint32_t frames);
// The display transform (display.inc, DESIGN.md "Display transform"): exposure and a tone-map curve over a finalised mode-0 frame of n pixels,
// in place, behind the finaliser and before the render scale and the 2D layer.  Manual exposure: launch_display_apply alone (frame_e null).
// Automatic: hist (into 256 zeroed words), resolve
// (one workgroup: the owner's record `state` = (E, E*, q, N) from the counts and the record before, this frame's E into *frame_e, the
// counts into hist_copy, the 256 words zeroed again), apply (frame_e = what resolve wrote).
struct DisplayParams {
    uint32_t curve = 0;         // option "tonemap": 0 off, 1 exposure only, 2 extended Reinhard, 3 ACES fit
    float exposure = 1.0f;      // "exposure"
    float white = 4.0f;         // "tonemap_white"
    uint32_t automatic = 0;     // "auto_exposure"
    float key = 0.18f;          // "exposure_key"
    float exposure_min = 1.0f / 64.0f, exposure_max = 64.0f;
    uint32_t low = 50, high = 95; // "exposure_low", "exposure_high": percent
    float speed = 0.125f;       // "exposure_speed"
};
constexpr uint32_t kDisplayStateWords = 4;      // the owner's record; the 256 counts it was resolved from follow it
constexpr uint32_t kDisplayHistWords = 256 + 4; // a slot's histogram, then its latest frame's E
void launch_display_hist(hipStream_t s, const float4* frame, uint64_t n, uint32_t* hist);
void launch_display_resolve(hipStream_t s, const DisplayParams& d, bool has_prev, uint32_t* hist, uint32_t* state, float* frame_e, uint32_t* hist_copy);
void launch_display_apply(hipStream_t s, const DisplayParams& d, const float* frame_e, float4* frame, uint64_t n);
void launch_eval_shading(hipStream_t s, const SceneDev& sc, const CameraParams& cam, int op, uint32_t n, const float* in, float* out);
void launch_query_closest(hipStream_t s, const SceneDev& sc, const float* origins, const float* directions, float t_min, float t_max, uint64_t n,
                          rfw_hip_hit* hits, uint32_t* depth = nullptr /* optional: nodes visited per ray */);
void launch_query_any(hipStream_t s, const SceneDev& sc, const float* origins, const float* directions, float t_min, const float* t_max, uint64_t n,
                      uint8_t* occluded, uint32_t* depth = nullptr /* optional: nodes visited per ray */);

} // namespace rfwhip
