// example_animated.cpp — the reference's `examples/animated` (examples/animated/src/main.rs) as a headless C++ program on the MI355X
// backend: a scene (a glTF file, or the synthetic atrium), a grid of icosphere instances that bounce every frame (bounce_spheres,
// main.rs:197-219), animated glTF models placed the way the reference places its two CesiumMan graphs (main.rs:79-103; `--actor`, up to
// twice) and the animation timer system (set_animation_timers, main.rs:221-223: Scene::set_animations_time every frame -> joint matrices
// -> skinning and BLAS refit on the device), driven exactly the way rfw drives a backend — synchronize_system, then render_system, every
// frame (rfw/src/system/mod.rs:19-206, rfw/src/lib.rs:411-430) — through the rfw::Backend interface of rfw_host.hpp.
//
// Where the reference presents to a window, this program downloads the presented (Bgra8UnormSrgb) frame of every frame into a ring of
// pinned host buffers without stalling the frames in flight, and writes the last one as a PPM image.
//
//   example_animated [--gltf scene.glb | scene.obj] [--actor animated.gltf]... [--frames N] [--size WxH] [--spheres NXxNZ] [--path-length L] [--denoise K] [--scale S] [--tonemap K [--auto-exposure]] [--material-maps] [--hud] [--out last.ppm]
//
// --denoise K (off by default) finalises every frame with K a-trous passes and a history of 16 samples that follows the bouncing
// instances and the skinned actor (options "denoise", "denoise_temporal", "denoise_motion", "denoise_deform"): every frame here is a new
// image of one sample per pixel.
// --tonemap K (off by default) passes every frame through the display transform (option "tonemap": 1 exposure only, 2 extended Reinhard,
// 3 ACES fit), --auto-exposure adapts the exposure to the frames' luminance from frame to frame (option "auto_exposure"); the exposure the
// last frame was shown with is printed.
// --material-maps (off by default) has the path tracer honour the materials' metallic-roughness, sheen and emissive maps (option
// "material_maps"); how many of the scene's materials have such a map that is live (its texture exists; an emissive map only on a material no
// colour component of which exceeds 1) is printed.
// --hud (off by default) draws the frame counter and the frame time over the image the way rfw-font draws the reference's FPS counter: one
// atlas texture (white, the glyphs in alpha, one mip level), one 2D mesh of glyph quads rewritten every frame, one 2D instance with the
// pixel-space matrix, and the frame's Camera2D view (line 1: "frame N", line 2: "T ms" of the frame before).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "rfw_host.hpp"

int main(int argc, char** argv)
{
    std::string gltf, out = "example_animated.ppm";
    std::vector<std::string> actors;
    uint32_t frames = 240, width = 1280, height = 720, nx = 100, nz = 100, path_length = 2, denoise = 0, tonemap = 0;
    bool hud = false, auto_exposure = false, material_maps = false;
    double scale = 1.0; // rfw's Settings::scale_mode = Custom(S): traced at size x S, presented at size
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--gltf") gltf = next();
        else if (a == "--actor") actors.push_back(next());
        else if (a == "--frames") frames = (uint32_t)std::atoi(next());
        else if (a == "--size") std::sscanf(next(), "%ux%u", &width, &height);
        else if (a == "--spheres") std::sscanf(next(), "%ux%u", &nx, &nz);
        else if (a == "--path-length") path_length = (uint32_t)std::atoi(next());
        else if (a == "--denoise") denoise = (uint32_t)std::atoi(next());
        else if (a == "--scale") scale = std::atof(next());
        else if (a == "--tonemap") tonemap = (uint32_t)std::atoi(next());
        else if (a == "--auto-exposure") auto_exposure = true;
        else if (a == "--material-maps") material_maps = true;
        else if (a == "--hud") hud = true;
        else if (a == "--out") out = next();
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (!width || !height || !frames) { std::fprintf(stderr, "bad --size / --frames\n"); return 2; }
    try {
        rfw::Scene scene;
        rfw::Camera3D camera;
        if (!gltf.empty()) {
            std::string err;
            const bool obj = gltf.size() > 4 && gltf.compare(gltf.size() - 4, 4, ".obj") == 0; // Scene::load picks the loader by extension
            if (!(obj ? rfw::load_obj(gltf, scene, err) : rfw::load_gltf(gltf, scene, &camera, err))) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        } else {
            rfw::build_atrium(scene, camera, 262267, 0xC0FFEE);
        }
        for (size_t k = 0; k < actors.size(); k++) { // main.rs:84-103: the first graph scaled by 3, the second moved to x = -3, both turned by 180 degrees about y
            std::string err;
            if (k > 0 && actors[k] == actors[0]) scene.instantiate_graph(scene.graphs.size() - k); // add_3d(&descriptor) again: same meshes, new instances and skins
            else if (!rfw::load_gltf(actors[k], scene, nullptr, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
            const double turn[4] = {0.0, 1.0, 0.0, 6.123233995736766e-17}; // quaternion of a half turn about y
            const double t0[3] = {0, 0, 0}, t1[3] = {-3.0 * (double)k, 0, 0}, s3[3] = {3, 3, 3}, s1[3] = {1, 1, 1};
            scene.graphs.back().set_root_transform(scene, k == 0 ? t0 : t1, turn, k == 0 ? s3 : s1);
        }
        scene.set_animations_time(0.0); // main.rs:112
        camera.aspect_ratio = (float)width / (float)height;
        const float spacing = 0.28f;
        rfw::add_sphere_grid(scene, nx, nz, spacing);
        const uint32_t grid_mesh = scene.meshes_3d.rbegin()->first;

        uint32_t hud_mesh = 0;
        int32_t hud_atlas = -1;
        const rfw::Camera2D camera_2d = rfw::Camera2D::from_width_height(width, height);
        if (hud) {
            hud_atlas = (int32_t)scene.textures.size();
            scene.textures.push_back(rfw::hud_font_atlas());
            scene.textures_changed = true;
            rfw::Mesh2D text;
            text.tex_id = hud_atlas;
            hud_mesh = scene.add_2d_mesh(text);
            scene.add_2d_instance(hud_mesh, rfw::hud_pixel_matrix(width, height));
        }

        rfw_hip_options opt;
        std::memset(&opt, 0, sizeof(opt));
        opt.struct_size = sizeof(opt);
        opt.device = -1;
        opt.max_path_length = path_length;
        opt.world = 1;
        opt.frames_in_flight = 4; // one HIP stream per frame slot
        std::unique_ptr<rfw::HipBackend> renderer(rfw::HipBackend::init(width, height, scale, &opt));
        std::printf("window %ux%u, scale %g: traced at %ux%u\n", width, height, scale, renderer->render_width(), renderer->render_height());

        if (denoise)
            for (const auto& kv : {std::pair<const char*, double>{"denoise", (double)denoise}, {"denoise_temporal", 16.0}, {"denoise_motion", 1.0}, {"denoise_deform", 1.0}})
                if (rfw_hip_set_option(renderer->raw(), kv.first, kv.second) != RFW_HIP_OK) throw std::runtime_error(rfw_hip_last_error(renderer->raw()));

        if (tonemap)
            for (const auto& kv : {std::pair<const char*, double>{"tonemap", (double)tonemap}, {"auto_exposure", auto_exposure ? 1.0 : 0.0}})
                if (rfw_hip_set_option(renderer->raw(), kv.first, kv.second) != RFW_HIP_OK) throw std::runtime_error(rfw_hip_last_error(renderer->raw()));

        if (material_maps) {
            if (rfw_hip_set_option(renderer->raw(), "material_maps", 1.0) != RFW_HIP_OK) throw std::runtime_error(rfw_hip_last_error(renderer->raw()));
            const int32_t n_tex = (int32_t)scene.textures.size();
            auto exists = [&](int32_t t) { return t >= 0 && t < n_tex; };
            uint32_t live = 0;
            for (const rfw::Material& m : scene.materials)
                if (exists(m.metallic_roughness_tex) || exists(m.sheen_tex) || (exists(m.emissive_tex) && !(m.color[0] > 1.0f || m.color[1] > 1.0f || m.color[2] > 1.0f))) live++;
            std::printf("material maps: %u of %zu materials have a live metallic-roughness, sheen or emissive map\n", live, scene.materials.size());
        }

        const uint64_t px = (uint64_t)width * height;
        std::vector<uint32_t*> ring(8, nullptr); // presented frames land here, 8 frames of slack
        for (uint32_t*& p : ring)
            if (!(p = (uint32_t*)rfw_hip_host_alloc(px * 4))) throw std::runtime_error("rfw_hip_host_alloc failed");

        rfw::synchronize_system(scene, *renderer); // first synchronize: uploads and builds everything
        const auto t0 = std::chrono::steady_clock::now();
        uint64_t rays = 0;
        auto t_prev = t0;
        double ms_prev = 0.0;
        for (uint32_t f = 0; f < frames; f++) {
            if (hud) { // the glyph mesh of this frame
                const float white[4] = {1, 1, 1, 1};
                const float scale = width >= 640 ? 2.0f : 1.0f;
                char line[64];
                rfw::Mesh2D text;
                text.tex_id = hud_atlas;
                std::snprintf(line, sizeof(line), "frame %u", f);
                rfw::hud_append_text(text, line, 0.0f, 1.0f, scale, white);
                std::snprintf(line, sizeof(line), "%.2f ms", ms_prev);
                rfw::hud_append_text(text, line, 0.0f, 1.0f + 9.0f * scale, scale, white);
                scene.set_2d_mesh(hud_mesh, text);
            }
            rfw::animate_sphere_grid(scene, grid_mesh, nx, nz, spacing, (float)f / 60.0f); // bounce_spheres at 60 Hz
            scene.set_animations_time((double)f / 60.0);                                   // set_animation_timers
            rfw::synchronize_system(scene, *renderer);                                    // changed instance lists -> TLAS of this frame
            if (hud) rfw::render_system(camera, camera_2d, width, height, *renderer);
            else rfw::render_system(camera, width, height, *renderer);
            const auto t_now = std::chrono::steady_clock::now();
            ms_prev = std::chrono::duration<double, std::milli>(t_now - t_prev).count();
            t_prev = t_now;
            uint32_t* dst = ring[f % ring.size()];
            if (f >= ring.size() && rfw_hip_wait_download(renderer->raw(), dst) != RFW_HIP_OK) throw std::runtime_error(rfw_hip_last_error(renderer->raw()));
            if (rfw_hip_download_frame(renderer->raw(), 2, 0, (float*)dst, px) != RFW_HIP_OK) throw std::runtime_error(rfw_hip_last_error(renderer->raw()));
        }
        if (rfw_hip_wait_downloads(renderer->raw()) != RFW_HIP_OK) throw std::runtime_error(rfw_hip_last_error(renderer->raw()));
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        rfw_hip_frame_stats st;
        std::memset(&st, 0, sizeof(st));
        if (rfw_hip_get_frame_stats(renderer->raw(), &st) == RFW_HIP_OK) rays = st.primary_rays + st.extension_rays + st.shadow_rays;
        std::printf("%u frames of %ux%u, %llu triangles, %u animated instances: %.2f ms per frame (%.0f frames/s), ~%.0f Mrays/s, every frame presented to host memory\n",
                    frames, width, height, (unsigned long long)scene.triangle_count(), nx * nz, secs / frames * 1e3, frames / secs,
                    (double)rays * frames / secs / 1e6);

        if (tonemap) { // what the display transform applied to the last frame
            float state[4] = {};
            uint64_t got = 0;
            if (rfw_hip_debug_read(renderer->raw(), "display_state", state, sizeof(state), &got) != RFW_HIP_OK) throw std::runtime_error(rfw_hip_last_error(renderer->raw()));
            if (got == sizeof(state)) std::printf("tonemap %u, %s exposure: the last frame was shown with exposure %.6g\n", tonemap, auto_exposure ? "automatic" : "manual", state[0]);
        }

        const uint32_t* last = ring[(frames - 1) % ring.size()];
        if (FILE* fp = std::fopen(out.c_str(), "wb")) {
            std::fprintf(fp, "P6\n%u %u\n255\n", width, height);
            std::vector<uint8_t> row(3 * (size_t)width);
            for (uint32_t y = 0; y < height; y++) {
                for (uint32_t x = 0; x < width; x++) {
                    const uint32_t c = last[(size_t)y * width + x]; // B, G, R, A in memory order
                    row[3 * x] = (uint8_t)(c >> 16); row[3 * x + 1] = (uint8_t)(c >> 8); row[3 * x + 2] = (uint8_t)c;
                }
                std::fwrite(row.data(), 1, row.size(), fp);
            }
            std::fclose(fp);
            std::printf("last frame -> %s\n", out.c_str());
        }
        for (uint32_t* p : ring) rfw_hip_host_free(p);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "example_animated: %s\n", e.what());
        return 1;
    }
    return 0;
}
