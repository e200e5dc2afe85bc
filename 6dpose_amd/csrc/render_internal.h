// Private view of lm_mesh shared by render.cpp, detector_bank.cpp and pipeline.cpp (not part of the C ABI).
#pragma once
#include "../../include/amd_linemod.h"
#include "dev_buf.h"
#include "render_kernels.h"

struct lm_mesh {
    int device = 0;
    int nv = 0, nf = 0;
    DevStream s;                           // before every buffer below: they die first (dev_buf.h)
    DevBuf<float> d_v, d_n;
    DevBuf<uint8_t> d_c;
    DevBuf<int32_t> d_f;
    // render scratch / results of the last call (device)
    DevBuf<lm::ViewParams> d_views;
    DevBuf<lm::ProjVtx> d_pv;
    DevBuf<unsigned long long> d_zbuf;
    DevBuf<uint16_t> d_depth;
    DevBuf<uint8_t> d_rgb;
    int last_W = 0, last_H = 0, last_count = 0;
    // pose-error scratch (pose_error.cpp): resident scene depth, pair parameters, per-block partials (bytes: each metric casts them to its records)
    DevBuf<float> d_scene;
    DevBuf<uint8_t> d_pe_pairs, d_pe_partial;
    // texture (lm_mesh_set_texcoords / lm_mesh_set_texture) and per-view surface colours of the last shaded render
    DevBuf<float> d_uv;                    // [nv][2]
    DevBuf<uint32_t> d_tex;                // [tex_h][tex_w] r | g << 8 | b << 16
    int tex_w = 0, tex_h = 0;
    DevBuf<uint32_t> d_view_surf;
    // overlay scratch / results (lm_mesh_overlay, held by the first mesh of the call)
    DevBuf<lm::OverlayLayer> d_ov_layers;
    DevBuf<uint8_t> d_ov_frame;
    DevBuf<uint16_t> d_ov_scene;
    DevBuf<uint8_t> d_ov_rgb;
    DevBuf<int8_t> d_ov_index;
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
