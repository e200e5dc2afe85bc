// lm_mesh — triangle meshes resident in HBM and their rendering into depth / colour images:
// the job pysixd's OpenGL renderer does for the reference driver (linemod_and_levelup_test.py:206-215 training
// views, :352 depth_ren of a match).  PLY reading follows pysixd/inout.py:load_ply (ascii and
// binary_little_endian; x y z [nx ny nz] [red green blue], triangular faces).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "render_internal.h"

using namespace lm;

extern "C" int lm_mesh_create(int device, const float* vertices, const float* normals, const uint8_t* colors, int nv, const int32_t* faces,
                              int nf, lm_mesh** out) {
    if (!out || !vertices || !faces || nv <= 0 || nf <= 0) return lm_set_error(LM_ERR_INVALID, "null / empty mesh");
    *out = nullptr;
    for (int i = 0; i < 3 * nf; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return lm_set_error(LM_ERR_INVALID, "face index %d out of range", faces[i]);
    if (int rc = lm_open_device(device)) return rc;
    lm_mesh* m = new lm_mesh();
    m->device = device; m->nv = nv; m->nf = nf;
    auto upload = [](auto& buf, const auto* src, size_t n) -> int {
        int rc = buf.ensure(n);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(buf.p, src, n * sizeof(*src), hipMemcpyHostToDevice));
        return LM_OK;
    };
    int rc = m->s.ensure(hipStreamNonBlocking);
    if (!rc) rc = upload(m->d_v, vertices, (size_t)nv * 3);
    if (!rc) rc = upload(m->d_f, faces, (size_t)nf * 3);
    if (!rc && normals) rc = upload(m->d_n, normals, (size_t)nv * 3);
    if (!rc && colors) rc = upload(m->d_c, colors, (size_t)nv * 3);
    if (rc) { lm_mesh_destroy(m); return rc; }                        // the message is the failed step's
    *out = m;
    return LM_OK;
}

extern "C" void lm_mesh_destroy(lm_mesh* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->s) (void)hipStreamSynchronize(m->s);
    delete m;                                                         // every buffer, then the stream: device selected, stream idle
}

extern "C" int lm_mesh_counts(const lm_mesh* m, int* nv, int* nf) {
    if (!m) return lm_set_error(LM_ERR_INVALID, "null mesh");
    if (nv) *nv = m->nv;
    if (nf) *nf = m->nf;
    return LM_OK;
}

// ---- PLY (pysixd/inout.py:load_ply) -----------------------------------------------------------------
namespace {
struct Prop { std::string name, type, list_count, list_item; bool is_list = false; };
int type_size(const std::string& t) {
    if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
    if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
    if (t == "int" || t == "uint" || t == "float" || t == "int32" || t == "uint32" || t == "float32") return 4;
    if (t == "double" || t == "float64") return 8;
    return 0;
}
double read_bin(const unsigned char* p, const std::string& t) {
    if (t == "char" || t == "int8") return (double)*(const signed char*)p;
    if (t == "uchar" || t == "uint8") return (double)*p;
    if (t == "short" || t == "int16") { int16_t v; memcpy(&v, p, 2); return v; }
    if (t == "ushort" || t == "uint16") { uint16_t v; memcpy(&v, p, 2); return v; }
    if (t == "int" || t == "int32") { int32_t v; memcpy(&v, p, 4); return v; }
    if (t == "uint" || t == "uint32") { uint32_t v; memcpy(&v, p, 4); return v; }
    if (t == "float" || t == "float32") { float v; memcpy(&v, p, 4); return v; }
    double v; memcpy(&v, p, 8); return v;
}
}  // namespace

extern "C" int lm_mesh_load_ply(int device, const char* path, lm_mesh** out) {
    if (!path || !out) return lm_set_error(LM_ERR_INVALID, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return lm_set_error(LM_ERR_IO, "cannot open %s", path);
    std::vector<unsigned char> buf;
    {
        fseek(f, 0, SEEK_END);
        long sz = ftell(f);
        fseek(f, 0, SEEK_SET);
        buf.resize(sz > 0 ? (size_t)sz : 0);
        if (sz > 0 && fread(buf.data(), 1, (size_t)sz, f) != (size_t)sz) { fclose(f); return lm_set_error(LM_ERR_IO, "short read of %s", path); }
        fclose(f);
    }
    size_t pos = 0;
    auto next_line = [&](std::string& line) {
        if (pos >= buf.size()) return false;
        size_t e = pos;
        while (e < buf.size() && buf[e] != '\n') ++e;
        line.assign((const char*)&buf[pos], e - pos);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        pos = e + 1;
        return true;
    };
    std::string line;
    if (!next_line(line) || line != "ply") return lm_set_error(LM_ERR_IO, "%s is not a PLY file", path);
    bool ascii = true;
    int nv = 0, nf = 0;
    std::vector<Prop> vprops, fprops;
    std::string cur;
    while (next_line(line)) {
        if (line == "end_header") break;
        char a[64] = {0}, b[64] = {0}, c[64] = {0}, d[64] = {0}, e[64] = {0};
        int n = sscanf(line.c_str(), "%63s %63s %63s %63s %63s", a, b, c, d, e);
        if (n >= 2 && !strcmp(a, "format")) {
            if (!strcmp(b, "ascii")) ascii = true;
            else if (!strcmp(b, "binary_little_endian")) ascii = false;
            else return lm_set_error(LM_ERR_IO, "unsupported PLY format '%s'", b);
        } else if (n >= 3 && !strcmp(a, "element")) {
            cur = b;
            if (cur == "vertex") nv = atoi(c);
            else if (cur == "face") nf = atoi(c);
        } else if (n >= 3 && !strcmp(a, "property")) {
            Prop p;
            if (!strcmp(b, "list")) { p.is_list = true; p.list_count = c; p.list_item = d; p.name = e; }
            else { p.type = b; p.name = c; }
            if (cur == "vertex") vprops.push_back(p);
            else if (cur == "face") fprops.push_back(p);
        }
    }
    if (nv <= 0 || nf <= 0) return lm_set_error(LM_ERR_IO, "%s: no vertices / faces", path);
    int ix = -1, iy = -1, iz = -1, inx = -1, iny = -1, inz = -1, ir = -1, ig = -1, ib = -1, itu = -1, itv = -1;
    for (size_t i = 0; i < vprops.size(); ++i) {
        const std::string& nm = vprops[i].name;
        if (vprops[i].is_list) return lm_set_error(LM_ERR_IO, "%s: list property on vertices", path);
        if (nm == "x") ix = (int)i; else if (nm == "y") iy = (int)i; else if (nm == "z") iz = (int)i;
        else if (nm == "nx") inx = (int)i; else if (nm == "ny") iny = (int)i; else if (nm == "nz") inz = (int)i;
        else if (nm == "red") ir = (int)i; else if (nm == "green") ig = (int)i; else if (nm == "blue") ib = (int)i;
        else if (nm == "texture_u") itu = (int)i; else if (nm == "texture_v") itv = (int)i;     // inout.py:249-293
    }
    if (ix < 0 || iy < 0 || iz < 0) return lm_set_error(LM_ERR_IO, "%s: vertices without x/y/z", path);
    const bool has_n = inx >= 0 && iny >= 0 && inz >= 0, has_c = ir >= 0 && ig >= 0 && ib >= 0;
    std::vector<float> V((size_t)nv * 3), N(has_n ? (size_t)nv * 3 : 0);
    std::vector<uint8_t> C(has_c ? (size_t)nv * 3 : 0);
    const bool has_uv = itu >= 0 && itv >= 0;
    std::vector<float> UV(has_uv ? (size_t)nv * 2 : 0);
    std::vector<int32_t> F;
    F.reserve((size_t)nf * 3);
    std::vector<double> vals(vprops.size());
    if (ascii) {
        const char* p = (const char*)buf.data() + pos;
        const char* end = (const char*)buf.data() + buf.size();
        auto num = [&](double& v) {
            while (p < end && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) ++p;
            if (p >= end) return false;
            char* q = nullptr;
            v = strtod(p, &q);
            if (q == p) return false;
            p = q;
            return true;
        };
        for (int i = 0; i < nv; ++i) {
            for (size_t k = 0; k < vprops.size(); ++k)
                if (!num(vals[k])) return lm_set_error(LM_ERR_IO, "%s: truncated vertex list", path);
            V[3 * (size_t)i] = (float)vals[ix]; V[3 * (size_t)i + 1] = (float)vals[iy]; V[3 * (size_t)i + 2] = (float)vals[iz];
            if (has_n) { N[3 * (size_t)i] = (float)vals[inx]; N[3 * (size_t)i + 1] = (float)vals[iny]; N[3 * (size_t)i + 2] = (float)vals[inz]; }
            if (has_c) { C[3 * (size_t)i] = (uint8_t)vals[ir]; C[3 * (size_t)i + 1] = (uint8_t)vals[ig]; C[3 * (size_t)i + 2] = (uint8_t)vals[ib]; }
            if (has_uv) { UV[2 * (size_t)i] = (float)vals[itu]; UV[2 * (size_t)i + 1] = (float)vals[itv]; }
        }
        for (int i = 0; i < nf; ++i) {
            for (const Prop& fp : fprops) {
                double cnt;
                if (!fp.is_list) { if (!num(cnt)) return lm_set_error(LM_ERR_IO, "%s: truncated face list", path); continue; }
                if (!num(cnt)) return lm_set_error(LM_ERR_IO, "%s: truncated face list", path);
                std::vector<int32_t> idx((size_t)cnt);
                for (int k = 0; k < (int)cnt; ++k) { double v; if (!num(v)) return lm_set_error(LM_ERR_IO, "%s: truncated face list", path); idx[k] = (int32_t)v; }
                if (fp.name == "vertex_indices" || fp.name == "vertex_index") {
                    if ((int)cnt != 3) return lm_set_error(LM_ERR_IO, "%s: only triangular faces are supported (inout.py:load_ply)", path);
                    F.insert(F.end(), idx.begin(), idx.end());
                }
            }
        }
    } else {
        const unsigned char* p = buf.data() + pos;
        const unsigned char* end = buf.data() + buf.size();
        for (int i = 0; i < nv; ++i) {
            for (size_t k = 0; k < vprops.size(); ++k) {
                const int ts = type_size(vprops[k].type);
                if (!ts || p + ts > end) return lm_set_error(LM_ERR_IO, "%s: truncated / unknown vertex data", path);
                vals[k] = read_bin(p, vprops[k].type);
                p += ts;
            }
            V[3 * (size_t)i] = (float)vals[ix]; V[3 * (size_t)i + 1] = (float)vals[iy]; V[3 * (size_t)i + 2] = (float)vals[iz];
            if (has_n) { N[3 * (size_t)i] = (float)vals[inx]; N[3 * (size_t)i + 1] = (float)vals[iny]; N[3 * (size_t)i + 2] = (float)vals[inz]; }
            if (has_c) { C[3 * (size_t)i] = (uint8_t)vals[ir]; C[3 * (size_t)i + 1] = (uint8_t)vals[ig]; C[3 * (size_t)i + 2] = (uint8_t)vals[ib]; }
            if (has_uv) { UV[2 * (size_t)i] = (float)vals[itu]; UV[2 * (size_t)i + 1] = (float)vals[itv]; }
        }
        for (int i = 0; i < nf; ++i) {
            for (const Prop& fp : fprops) {
                if (!fp.is_list) { const int ts = type_size(fp.type); if (!ts || p + ts > end) return lm_set_error(LM_ERR_IO, "%s: truncated face data", path); p += ts; continue; }
                const int cs = type_size(fp.list_count), is = type_size(fp.list_item);
                if (!cs || !is || p + cs > end) return lm_set_error(LM_ERR_IO, "%s: truncated face data", path);
                const int cnt = (int)read_bin(p, fp.list_count);
                p += cs;
                if (cnt < 0 || p + (size_t)cnt * is > end) return lm_set_error(LM_ERR_IO, "%s: truncated face data", path);
                const bool vi = fp.name == "vertex_indices" || fp.name == "vertex_index";
                if (vi && cnt != 3) return lm_set_error(LM_ERR_IO, "%s: only triangular faces are supported (inout.py:load_ply)", path);
                for (int k = 0; k < cnt; ++k) { if (vi) F.push_back((int32_t)read_bin(p, fp.list_item)); p += is; }
            }
        }
    }
    if ((int)(F.size() / 3) != nf) return lm_set_error(LM_ERR_IO, "%s: %d faces announced, %d read", path, nf, (int)(F.size() / 3));
    int rc = lm_mesh_create(device, V.data(), has_n ? N.data() : nullptr, has_c ? C.data() : nullptr, nv, F.data(), nf, out);
    if (rc || !has_uv) return rc;
    if ((rc = lm_mesh_set_texcoords(*out, UV.data(), nv))) { lm_mesh_destroy(*out); *out = nullptr; }
    return rc;
}

// ---- texture (renderer.py:316-321; inout.py:249-293 texture_u / texture_v) ----------------------------
extern "C" int lm_mesh_set_texcoords(lm_mesh* m, const float* uv, int count) {
    if (!m || !uv) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (count != m->nv) return lm_set_error(LM_ERR_INVALID, "%d texture coordinates for %d vertices", count, m->nv);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->s));
    int rc = m->d_uv.ensure((size_t)m->nv * 2);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(m->d_uv.p, uv, (size_t)m->nv * 2 * sizeof(float), hipMemcpyHostToDevice));
    return LM_OK;
}

extern "C" int lm_mesh_set_texture(lm_mesh* m, const uint8_t* rgb, int width, int height) {
    if (!m || !rgb) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (width <= 0 || height <= 0 || width > 16384 || height > 16384) return lm_set_error(LM_ERR_INVALID, "unsupported texture size %dx%d", width, height);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->s));
    const size_t n = (size_t)width * height;
    std::vector<uint32_t> texels(n);                                   // 4-byte texels: one dword load per lookup
    for (size_t i = 0; i < n; ++i) texels[i] = (uint32_t)rgb[3 * i] | ((uint32_t)rgb[3 * i + 1] << 8) | ((uint32_t)rgb[3 * i + 2] << 16);
    m->d_tex.release(); m->tex_w = m->tex_h = 0;                      // exactly this size, not a grown buffer
    int rc = m->d_tex.ensure(n);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(m->d_tex.p, texels.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    m->tex_w = width; m->tex_h = height;
    return LM_OK;
}

extern "C" int lm_mesh_texture_info(const lm_mesh* m, int* has_texcoords, int* width, int* height) {
    if (!m) return lm_set_error(LM_ERR_INVALID, "null mesh");
    if (has_texcoords) *has_texcoords = m->d_uv.p != nullptr;
    if (width) *width = m->tex_w;
    if (height) *height = m->tex_h;
    return LM_OK;
}

extern "C" void lm_render_options_init(lm_render_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->size = (uint32_t)sizeof(*o);
    o->shading = LM_SHADING_PHONG;
    o->ambient = 0.8f; o->ssaa = 4; o->clip_near = 10.f; o->clip_far = 10000.f;
}

static bool pack_colour(const float* c, uint32_t* out) {
    uint32_t v = 0;
    for (int k = 0; k < 3; ++k) {
        if (!(c[k] >= 0.f && c[k] <= 1.f)) return false;               // NaN fails too
        v |= (uint32_t)lrintf(c[k] * 255.f) << (8 * k);
    }
    *out = v;
    return true;
}

int lm_parse_render_options(const lm_mesh* m, const lm_render_options* o, lm_shade_opts* out) {
    if (!m || !o || !out) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (o->size != sizeof(lm_render_options)) return lm_set_error(LM_ERR_INVALID, "lm_render_options.size is %u, this library expects %u", o->size, (unsigned)sizeof(lm_render_options));
    if (o->shading != LM_SHADING_PHONG && o->shading != LM_SHADING_FLAT) return lm_set_error(LM_ERR_INVALID, "unknown shading %d", o->shading);
    lm_shade_opts r;
    r.flat = o->shading == LM_SHADING_FLAT;
    r.use_texture = o->use_texture != 0;
    if (r.use_texture && (!m->d_uv.p || !m->d_tex.p)) return lm_set_error(LM_ERR_INVALID, "texture requested but the mesh has %s", !m->d_uv.p ? "no texture coordinates" : "no texture image");
    r.has_surf = o->has_surf_color != 0;
    if (r.has_surf && !pack_colour(o->surf_color, &r.surf)) return lm_set_error(LM_ERR_INVALID, "surf_color outside [0, 1]");
    if (!pack_colour(o->bg_color, &r.bg) || !(o->bg_color[3] >= 0.f && o->bg_color[3] <= 1.f)) return lm_set_error(LM_ERR_INVALID, "bg_color outside [0, 1]");
    if (!(o->ambient >= 0.f)) return lm_set_error(LM_ERR_INVALID, "ambient weight must be >= 0");
    r.ambient = o->ambient; r.ssaa = o->ssaa; r.clip_near = o->clip_near; r.clip_far = o->clip_far;
    *out = r;
    return LM_OK;
}

// ---- rendering -----------------------------------------------------------------------------------------
static int render_device(lm_mesh* m, int count, int W, int H, const float* Ks, const float* Rs, const float* ts, float clip_near,
                         float clip_far, float ambient, int ssaa, bool want_depth, bool want_rgb, const lm_shade_opts* shade) {
    if (!m || count <= 0 || W <= 0 || H <= 0 || !Ks || !Rs || !ts) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (ssaa < 1 || ssaa > 8) return lm_set_error(LM_ERR_INVALID, "ssaa must be in 1..8");
    HIP_TRY(hipSetDevice(m->device));
    const size_t nview = (size_t)count;
    std::vector<ViewParams> hv(nview);
    for (int i = 0; i < count; ++i) {
        for (int k = 0; k < 9; ++k) { hv[i].K[k] = Ks[9 * i + k]; hv[i].R[k] = Rs[9 * i + k]; }
        for (int k = 0; k < 3; ++k) hv[i].t[k] = ts[3 * i + k];
    }
    const int smax = want_rgb ? ssaa : 1;
    int rc;
    if ((rc = m->d_views.ensure(nview))) return rc;
    if ((rc = m->d_pv.ensure(nview * m->nv))) return rc;
    if ((rc = m->d_zbuf.ensure(nview * W * H * smax * smax))) return rc;
    if (want_depth && (rc = m->d_depth.ensure(nview * W * H))) return rc;
    if (want_rgb && (rc = m->d_rgb.ensure(nview * W * H * 3))) return rc;
    if (want_rgb && shade && shade->view_surf) {
        if ((rc = m->d_view_surf.ensure(nview))) return rc;
        HIP_TRY(hipMemcpyAsync(m->d_view_surf.p, shade->view_surf, nview * sizeof(uint32_t), hipMemcpyHostToDevice, m->s));
    }
    HIP_TRY(hipMemcpyAsync(m->d_views.p, hv.data(), nview * sizeof(ViewParams), hipMemcpyHostToDevice, m->s));
    HIP_TRY(hipStreamSynchronize(m->s));                              // hv is a local
    MeshDev M{m->d_v.p, m->d_n.p, m->d_c.p, m->d_f.p, m->nv, m->nf};
    if (want_depth) {                                                 // the driver renders depth at the native resolution (:206-209)
        HIP_TRY(launch_project(M, m->d_views.p, count, 1, m->d_pv.p, m->s));
        HIP_TRY(launch_raster(M, m->d_pv.p, count, W, H, clip_near, clip_far, m->d_zbuf.p, m->s));
        HIP_TRY(launch_resolve_depth(m->d_zbuf.p, count, W, H, m->d_depth.p, m->s));
    }
    if (want_rgb) {                                                   // and colour at ssaa x, box-filtered (:212-216)
        HIP_TRY(launch_project(M, m->d_views.p, count, ssaa, m->d_pv.p, m->s));
        HIP_TRY(launch_raster(M, m->d_pv.p, count, W * ssaa, H * ssaa, clip_near, clip_far, m->d_zbuf.p, m->s));
        if (!shade) HIP_TRY(launch_resolve_rgb(M, m->d_pv.p, m->d_views.p, m->d_zbuf.p, count, W, H, ssaa, ambient, m->d_rgb.p, m->s));
        else {
            ShadeParams sp{};
            if (shade->use_texture) { sp.uv = m->d_uv.p; sp.tex = m->d_tex.p; sp.tex_w = m->tex_w; sp.tex_h = m->tex_h; }
            sp.view_surf = shade->view_surf ? m->d_view_surf.p : nullptr;
            sp.surf = shade->surf; sp.has_surf = shade->has_surf; sp.bg = shade->bg; sp.ambient = ambient; sp.flat = shade->flat;
            HIP_TRY(launch_resolve_shaded(M, m->d_pv.p, m->d_views.p, m->d_zbuf.p, count, W, H, ssaa, sp, m->d_rgb.p, m->s));
        }
    }
    m->last_W = W; m->last_H = H; m->last_count = count;
    return LM_OK;
}

int lm_mesh_render_device(lm_mesh* m, int count, int W, int H, const float* Ks, const float* Rs, const float* ts, float clip_near,
                          float clip_far, float ambient, int ssaa, bool want_depth, bool want_rgb) {
    return render_device(m, count, W, H, Ks, Rs, ts, clip_near, clip_far, ambient, ssaa, want_depth, want_rgb, nullptr);
}
int lm_mesh_render_device_shaded(lm_mesh* m, int count, int W, int H, const float* Ks, const float* Rs, const float* ts, const lm_shade_opts& o,
                                 bool want_depth, bool want_rgb) {
    if (o.use_texture && (!m || !m->d_uv.p || !m->d_tex.p)) return lm_set_error(LM_ERR_INVALID, "texture requested but none attached");
    return render_device(m, count, W, H, Ks, Rs, ts, o.clip_near, o.clip_far, o.ambient, o.ssaa, want_depth, want_rgb, &o);
}

extern "C" int lm_mesh_render(lm_mesh* m, int count, int width, int height, const float* Ks, const float* Rs, const float* ts,
                              float clip_near, float clip_far, float ambient, int ssaa, uint16_t* depth_out, uint8_t* rgb_out) {
    if (!depth_out && !rgb_out) return lm_set_error(LM_ERR_INVALID, "nothing to render into");
    // views in chunks that keep the ssaa id buffer below ~2 GB
    const size_t per_view = (size_t)width * height * (rgb_out ? (size_t)ssaa * ssaa : 1) * sizeof(unsigned long long);
    int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, ((size_t)2 << 30) / std::max<size_t>(per_view, 1)));
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int n = std::min(chunk, count - c0);
        int rc = lm_mesh_render_device(m, n, width, height, Ks + 9 * (size_t)c0, Rs + 9 * (size_t)c0, ts + 3 * (size_t)c0, clip_near, clip_far,
                                       ambient, ssaa, depth_out != nullptr, rgb_out != nullptr);
        if (rc) return rc;
        const size_t npx = (size_t)width * height;
        if (depth_out) HIP_TRY(hipMemcpyAsync(depth_out + (size_t)c0 * npx, m->d_depth.p, (size_t)n * npx * sizeof(uint16_t), hipMemcpyDeviceToHost, m->s));
        if (rgb_out) HIP_TRY(hipMemcpyAsync(rgb_out + (size_t)c0 * npx * 3, m->d_rgb.p, (size_t)n * npx * 3, hipMemcpyDeviceToHost, m->s));
        HIP_TRY(hipStreamSynchronize(m->s));
    }
    return LM_OK;
}

// render(model, im_size, K, R, t, clip_near, clip_far, texture, surf_color, bg_color, ambient_weight, shading) (renderer.py:306)
extern "C" int lm_mesh_render_ex(lm_mesh* m, int count, int width, int height, const float* Ks, const float* Rs, const float* ts,
                                 const lm_render_options* options, uint16_t* depth_out, uint8_t* rgb_out) {
    if (!depth_out && !rgb_out) return lm_set_error(LM_ERR_INVALID, "nothing to render into");
    lm_shade_opts o;
    int rc = lm_parse_render_options(m, options, &o);
    if (rc) return rc;
    if (count <= 0 || width <= 0 || height <= 0 || !Ks || !Rs || !ts) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (o.ssaa < 1 || o.ssaa > 8) return lm_set_error(LM_ERR_INVALID, "ssaa must be in 1..8");
    const size_t per_view = (size_t)width * height * (rgb_out ? (size_t)o.ssaa * o.ssaa : 1) * sizeof(unsigned long long);
    int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, ((size_t)2 << 30) / std::max<size_t>(per_view, 1)));
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int n = std::min(chunk, count - c0);
        rc = lm_mesh_render_device_shaded(m, n, width, height, Ks + 9 * (size_t)c0, Rs + 9 * (size_t)c0, ts + 3 * (size_t)c0, o, depth_out != nullptr,
                                          rgb_out != nullptr);
        if (rc) return rc;
        const size_t npx = (size_t)width * height;
        if (depth_out) HIP_TRY(hipMemcpyAsync(depth_out + (size_t)c0 * npx, m->d_depth.p, (size_t)n * npx * sizeof(uint16_t), hipMemcpyDeviceToHost, m->s));
        if (rgb_out) HIP_TRY(hipMemcpyAsync(rgb_out + (size_t)c0 * npx * 3, m->d_rgb.p, (size_t)n * npx * 3, hipMemcpyDeviceToHost, m->s));
        HIP_TRY(hipStreamSynchronize(m->s));
    }
    return LM_OK;
}

// ---- pose overlays (linemod_and_levelup_test.py:377-383, tools/vis_gt_poses.py:120-145) ------------------
extern "C" int lm_mesh_overlay(lm_mesh* const* meshes, int count, int width, int height, const uint8_t* rgb, const float* Ks, const float* Rs,
                               const float* ts, const float* surf_colors, const lm_render_options* options, const uint16_t* scene_depth,
                               int mode, uint8_t* rgb_out, int8_t* index_out) {
    if (!meshes || !rgb || !Ks || !Rs || !ts || !rgb_out || !index_out) return lm_set_error(LM_ERR_INVALID, "null argument");
    if (count < 1 || count > 127) return lm_set_error(LM_ERR_INVALID, "an overlay takes 1..127 poses (int8 index map), got %d", count);
    if (width <= 0 || height <= 0) return lm_set_error(LM_ERR_INVALID, "unsupported frame size %dx%d", width, height);
    if (mode != LM_OVERLAY_PAINTER && mode != LM_OVERLAY_NEAREST) return lm_set_error(LM_ERR_INVALID, "unknown overlay mode %d", mode);
    for (int i = 0; i < count; ++i) {
        if (!meshes[i]) return lm_set_error(LM_ERR_INVALID, "null mesh");
        if (meshes[i]->device != meshes[0]->device) return lm_set_error(LM_ERR_INVALID, "meshes live on different devices");
    }
    const size_t npx = (size_t)width * height;
    if ((size_t)count * npx * sizeof(unsigned long long) > ((size_t)2 << 30)) return lm_set_error(LM_ERR_INVALID, "overlay too large: %d poses at %dx%d", count, width, height);
    std::vector<uint32_t> surf(count, 0);
    if (surf_colors)
        for (int i = 0; i < count; ++i)
            if (!pack_colour(surf_colors + 3 * (size_t)i, &surf[i])) return lm_set_error(LM_ERR_INVALID, "surf_color outside [0, 1]");
    lm_mesh* m0 = meshes[0];
    HIP_TRY(hipSetDevice(m0->device));
    // one batch of renders per distinct mesh, each into that mesh's own buffers
    std::vector<OverlayLayer> layers(count);
    std::vector<char> done(count, 0);
    std::vector<float> K, R, T;
    std::vector<uint32_t> vs;
    for (int i = 0; i < count; ++i) {
        if (done[i]) continue;
        lm_mesh* m = meshes[i];
        lm_shade_opts o;
        int rc = lm_parse_render_options(m, options, &o);
        if (rc) return rc;
        if (o.ssaa != 1) return lm_set_error(LM_ERR_INVALID, "overlays render at ssaa 1 (colour and depth must cover the same pixels)");
        std::vector<int> mine;
        for (int j = i; j < count; ++j) if (meshes[j] == m) { mine.push_back(j); done[j] = 1; }
        const int n = (int)mine.size();
        K.resize(9 * (size_t)n); R.resize(9 * (size_t)n); T.resize(3 * (size_t)n); vs.resize(n);
        for (int k = 0; k < n; ++k) {
            memcpy(&K[9 * (size_t)k], Ks + 9 * (size_t)mine[k], 9 * sizeof(float));
            memcpy(&R[9 * (size_t)k], Rs + 9 * (size_t)mine[k], 9 * sizeof(float));
            memcpy(&T[3 * (size_t)k], ts + 3 * (size_t)mine[k], 3 * sizeof(float));
            vs[k] = surf[mine[k]];
        }
        o.view_surf = surf_colors ? vs.data() : nullptr;
        if ((rc = lm_mesh_render_device_shaded(m, n, width, height, K.data(), R.data(), T.data(), o, true, true))) return rc;
        HIP_TRY(hipStreamSynchronize(m->s));                           // vs is reused; the compose runs on m0's stream
        for (int k = 0; k < n; ++k) layers[mine[k]] = OverlayLayer{m->d_rgb.p + (size_t)k * npx * 3, m->d_depth.p + (size_t)k * npx};
    }
    int rc;
    if ((rc = m0->d_ov_layers.ensure(count))) return rc;
    if ((rc = m0->d_ov_frame.ensure(npx * 3))) return rc;
    if ((rc = m0->d_ov_rgb.ensure(npx * 3))) return rc;
    if ((rc = m0->d_ov_index.ensure(npx))) return rc;
    if (scene_depth && (rc = m0->d_ov_scene.ensure(npx))) return rc;
    HIP_TRY(hipMemcpyAsync(m0->d_ov_layers.p, layers.data(), (size_t)count * sizeof(OverlayLayer), hipMemcpyHostToDevice, m0->s));
    HIP_TRY(hipMemcpyAsync(m0->d_ov_frame.p, rgb, npx * 3, hipMemcpyHostToDevice, m0->s));
    if (scene_depth) HIP_TRY(hipMemcpyAsync(m0->d_ov_scene.p, scene_depth, npx * sizeof(uint16_t), hipMemcpyHostToDevice, m0->s));
    HIP_TRY(launch_overlay_compose(m0->d_ov_layers.p, count, m0->d_ov_frame.p, scene_depth ? m0->d_ov_scene.p : nullptr, (int)npx, mode == LM_OVERLAY_NEAREST,
                                   m0->d_ov_rgb.p, m0->d_ov_index.p, m0->s));
    HIP_TRY(hipMemcpyAsync(rgb_out, m0->d_ov_rgb.p, npx * 3, hipMemcpyDeviceToHost, m0->s));
    HIP_TRY(hipMemcpyAsync(index_out, m0->d_ov_index.p, npx, hipMemcpyDeviceToHost, m0->s));
    HIP_TRY(hipStreamSynchronize(m0->s));
    return LM_OK;
}
