// Times the colour render of lm_mesh on the device with hipEvents on the mesh's own stream: 64 views of a mesh at 640x480,
// ssaa 4, no host copy (lm_mesh_render_device).  Median / min / max of nine after two warm-up calls, one JSON line per mode.
// The default mode is the resolve kernel of lm_mesh_render; with -DHAVE_SHADED the modes of lm_mesh_render_ex follow.
// Build (from the repository root), then run with the library's directory on LD_LIBRARY_PATH:
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 [-DHAVE_SHADED] -I6dpose_amd/csrc profiles/render_shade_bench.cpp \
//         -L6dpose_amd -lamdlinemod -o render_shade_bench
//   ./render_shade_bench mesh.ply [label]
// The same source built against an older checkout (without -DHAVE_SHADED) times that checkout's default mode.
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "render_internal.h"

static const int kViews = 64, kW = 640, kH = 480, kSsaa = 4, kReps = 9, kWarm = 2;

template <class Fn>
static int time_mode(const char* label, const char* mode, lm_mesh* m, Fn&& call) {
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1;
    std::vector<float> ms;
    for (int i = 0; i < kWarm + kReps; ++i) {
        if (hipEventRecord(e0, m->s) != hipSuccess) return 1;
        if (call()) { fprintf(stderr, "%s: %s\n", mode, lm_last_error()); return 1; }
        if (hipEventRecord(e1, m->s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return 1;
        float t = 0.f;
        if (hipEventElapsedTime(&t, e0, e1) != hipSuccess) return 1;
        if (i >= kWarm) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"build\": \"%s\", \"mode\": \"%s\", \"views\": %d, \"size\": [%d, %d], \"ssaa\": %d, \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f}\n",
           label, mode, kViews, kW, kH, kSsaa, ms[ms.size() / 2], ms.front(), ms.back());
    fflush(stdout);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s mesh.ply [label]\n", argv[0]); return 2; }
    const char* label = argc > 2 ? argv[2] : "build";
    lm_mesh* m = nullptr;
    if (lm_mesh_load_ply(0, argv[1], &m)) { fprintf(stderr, "%s\n", lm_last_error()); return 1; }
    std::vector<float> K(9 * kViews), R(9 * kViews), T(3 * kViews);
    for (int i = 0; i < kViews; ++i) {
        const float k[9] = {572.4114f, 0, 325.2611f, 0, 573.57043f, 242.04899f, 0, 0, 1};
        const float a = 6.2831853f * i / kViews, c = cosf(a), s = sinf(a);
        const float r[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
        for (int j = 0; j < 9; ++j) { K[9 * i + j] = k[j]; R[9 * i + j] = r[j]; }
        T[3 * i] = 10.f * (i % 5 - 2); T[3 * i + 1] = 5.f * (i % 3 - 1); T[3 * i + 2] = 600.f;
    }
    int rc = time_mode(label, "default phong (lm_mesh_render)", m, [&] {
        return lm_mesh_render_device(m, kViews, kW, kH, K.data(), R.data(), T.data(), 10.f, 10000.f, 0.8f, kSsaa, false, true);
    });
#ifdef HAVE_SHADED
    int nv = 0, nf = 0;
    lm_mesh_counts(m, &nv, &nf);
    std::vector<float> uv(2 * (size_t)nv);
    for (int i = 0; i < nv; ++i) { uv[2 * i] = (float)(i % 97) / 96.f; uv[2 * i + 1] = (float)(i % 89) / 88.f; }
    std::vector<uint8_t> tex(512 * 512 * 3);
    for (size_t i = 0; i < tex.size(); ++i) tex[i] = (uint8_t)(i * 2654435761u >> 24);
    if (lm_mesh_set_texcoords(m, uv.data(), nv) || lm_mesh_set_texture(m, tex.data(), 512, 512)) { fprintf(stderr, "%s\n", lm_last_error()); return 1; }
    struct { const char* name; bool flat, tex, surf, bg; } modes[] = {{"phong (lm_mesh_render_ex)", false, false, false, false},
        {"flat", true, false, false, false}, {"phong + texture", false, true, false, false}, {"flat + texture", true, true, false, false},
        {"flat + surf_color + bg_color", true, false, true, true}};
    for (const auto& md : modes) {
        lm_shade_opts o;
        o.flat = md.flat; o.use_texture = md.tex; o.has_surf = md.surf; o.surf = 0x3366CCu; o.bg = md.bg ? 0x804020u : 0u;
        o.ssaa = kSsaa;
        rc |= time_mode(label, md.name, m, [&] { return lm_mesh_render_device_shaded(m, kViews, kW, kH, K.data(), R.data(), T.data(), o, false, true); });
    }
#endif
    lm_mesh_destroy(m);
    return rc;
}
