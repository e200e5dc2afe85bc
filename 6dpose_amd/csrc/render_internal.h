// Private view of lm_mesh shared by render.cpp, detector_bank.cpp and pipeline.cpp (not part of the C ABI).
#pragma once
#include "../../include/amd_linemod.h"
#include "render_kernels.h"

int lm_set_error(int code, const char* fmt, ...);
#ifndef HIP_TRY
#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return lm_set_error(LM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                                  __FILE__, __LINE__);                                        \
    } while (0)
#endif

struct lm_mesh {
    int device = 0;
    int nv = 0, nf = 0;
    hipStream_t s = nullptr;
    float* d_v = nullptr;
    float* d_n = nullptr;
    uint8_t* d_c = nullptr;
    int32_t* d_f = nullptr;
    // render scratch / results of the last call (device)
    lm::ViewParams* d_views = nullptr;
    lm::ProjVtx* d_pv = nullptr;
    unsigned long long* d_zbuf = nullptr;
    uint16_t* d_depth = nullptr;
    uint8_t* d_rgb = nullptr;
    size_t cap_views = 0, cap_pv = 0, cap_zbuf = 0, cap_depth = 0, cap_rgb = 0;
    int last_W = 0, last_H = 0, last_count = 0;
    // pose-error scratch (pose_error.cpp): resident scene depth, pair parameters, per-block partials
    float* d_scene = nullptr;
    void* d_pe_pairs = nullptr;
    void* d_pe_partial = nullptr;
    size_t cap_scene = 0, cap_pe_pairs = 0, cap_pe_partial = 0;
    // texture (lm_mesh_set_texcoords / lm_mesh_set_texture) and per-view surface colours of the last shaded render
    float* d_uv = nullptr;                 // [nv][2]
    uint32_t* d_tex = nullptr;             // [tex_h][tex_w] r | g << 8 | b << 16
    int tex_w = 0, tex_h = 0;
    uint32_t* d_view_surf = nullptr;
    size_t cap_view_surf = 0;
    // overlay scratch / results (lm_mesh_overlay, held by the first mesh of the call)
    lm::OverlayLayer* d_ov_layers = nullptr;
    uint8_t* d_ov_frame = nullptr;
    uint16_t* d_ov_scene = nullptr;
    uint8_t* d_ov_rgb = nullptr;
    int8_t* d_ov_index = nullptr;
    size_t cap_ov_layers = 0, cap_ov_frame = 0, cap_ov_scene = 0, cap_ov_rgb = 0, cap_ov_index = 0;
};

// Renders `count` views into the mesh's device buffers (d_depth [count][H][W], d_rgb [count][H][W][3]) on m->s; no host copy.
int lm_mesh_render_device(lm_mesh* m, int count, int W, int H, const float* Ks, const float* Rs, const float* ts, float clip_near,
                          float clip_far, float ambient, int ssaa, bool want_depth, bool want_rgb);

// A validated lm_render_options (render.cpp: lm_parse_render_options), colours packed r | g << 8 | b << 16.
struct lm_shade_opts {
    bool flat = false, use_texture = false, has_surf = false;
    uint32_t surf = 0, bg = 0;
    float ambient = 0.8f, clip_near = 10.f, clip_far = 10000.f;
    int ssaa = 4;
    const uint32_t* view_surf = nullptr;   // host, [count]: one surface colour per view (overlays)
};
int lm_parse_render_options(const lm_mesh* m, const lm_render_options* o, lm_shade_opts* out);
// lm_mesh_render_device with the resolve of the shading options (k_resolve_shaded).
int lm_mesh_render_device_shaded(lm_mesh* m, int count, int W, int H, const float* Ks, const float* Rs, const float* ts, const lm_shade_opts& o,
                                 bool want_depth, bool want_rgb);
