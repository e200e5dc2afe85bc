// Internal interface between render.cpp (host) and render.hip (kernels).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lm {

struct MeshDev {
    const float* v;      // [nv][3] model coordinates (mm)
    const float* n;      // [nv][3] vertex normals, may be null
    const uint8_t* c;    // [nv][3] vertex colours, may be null
    const int32_t* f;    // [nf][3]
    int nv, nf;
};
struct ViewParams {      // one view: OpenCV camera, p_cam = R v + t
    double K[9], R[9], t[3];
};
struct ProjVtx {
    double z;            // eye depth (mm)
    int sx, sy;          // screen position in 1/256 pixel
    int valid, pad;
};

[[nodiscard]] hipError_t launch_project(const MeshDev& M, const ViewParams* views, int count, int scale, ProjVtx* out, hipStream_t s);
[[nodiscard]] hipError_t launch_raster(const MeshDev& M, const ProjVtx* pv, int count, int Ws, int Hs, double clip_near, double clip_far,
                                       unsigned long long* zbuf, hipStream_t s);
[[nodiscard]] hipError_t launch_resolve_depth(const unsigned long long* zbuf, int count, int W, int H, uint16_t* depth, hipStream_t s);
[[nodiscard]] hipError_t launch_resolve_rgb(const MeshDev& M, const ProjVtx* pv, const ViewParams* views, const unsigned long long* zbuf, int count, int W, int H,
                                            int ssaa, float ambient, uint8_t* rgb, hipStream_t s);

// The resolve with the options of renderer.render beyond the default (render.hip, "shading options").  Colours are packed
// r | g << 8 | b << 16, 8 bits each.
struct ShadeParams {
    const float* uv;            // [nv][2] texture coordinates, null without a texture
    const uint32_t* tex;        // [tex_h][tex_w] texels, image row 0 first, null without a texture
    int tex_w, tex_h;
    const uint32_t* view_surf;  // [count] one surface colour per view, or null
    uint32_t surf;              // surface colour of every view (has_surf != 0, view_surf == null)
    int has_surf;
    uint32_t bg;                // colour of the supersamples no fragment covers
    float ambient;
    int flat;                   // 0: phong (interpolated vertex normals), 1: flat (face normal turned to the camera)
};
[[nodiscard]] hipError_t launch_resolve_shaded(const MeshDev& M, const ProjVtx* pv, const ViewParams* views, const unsigned long long* zbuf, int count, int W, int H,
                                               int ssaa, const ShadeParams& sp, uint8_t* rgb, hipStream_t s);

// Pose overlays: layer p of the composition is view p of some mesh's last render (colour and depth at the frame's size).
struct OverlayLayer {
    const uint8_t* rgb;         // [H][W][3]
    const uint16_t* depth;      // [H][W] mm, 0 = not covered
};
[[nodiscard]] hipError_t launch_overlay_compose(const OverlayLayer* layers, int count, const uint8_t* frame, const uint16_t* scene, int npx, int nearest,
                                                uint8_t* out_rgb, int8_t* out_index, hipStream_t s);

}  // namespace lm
