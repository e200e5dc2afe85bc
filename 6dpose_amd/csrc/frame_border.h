// Frames of any size: the border policy of a detector, the one rule that gives the aligned size of a source
// size, and the kernel that turns uploaded sources into the frame buffers of the aligned geometry (frame_border.hip).
// The size rule is plain host C++ with no dependency, so a CPU program can include this header alone.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace lm {

enum { kBorderStrict = 0, kBorderPad = 1, kBorderCrop = 2 };

// One side of a frame serves every level: level l has (v >> l) % T[l] == 0, and v halves L - 1 times without a remainder.
inline bool border_side_ok(int v, const int* T, int L) {
    if (v < 1 || v % (1 << (L - 1))) return false;
    for (int l = 0; l < L; ++l)
        if ((v >> l) < 1 || (v >> l) % T[l]) return false;
    return true;
}
// ... and both sides together: (rows * cols) % 16 == 0 at every level (LL.cpp:1136)
inline bool border_area_ok(int w, int h, int L) {
    for (int l = 0; l < L; ++l)
        if (((long long)(w >> l) * (h >> l)) % 16) return false;
    return true;
}
inline bool border_is_aligned(const int* T, int L, int W, int H) {
    return border_side_ok(W, T, L) && border_side_ok(H, T, L) && border_area_ok(W, H, L);
}

// The aligned size of a W x H source.  pad: the smallest Ha >= H, then the smallest Wa >= W; crop: the largest Ha <= H, then the largest
// Wa <= W, both at least 16; strict: the source itself.  False when there is none (crop: nothing of at least 16 fits; strict: W x H is
// not aligned; pad: beyond `limit`).
inline bool border_aligned_size(const int* T, int L, int policy, int W, int H, int* Wa, int* Ha, int limit = 1 << 20) {
    if (L < 1 || W < 1 || H < 1) return false;
    if (policy == kBorderStrict) {
        *Wa = W; *Ha = H;
        return border_is_aligned(T, L, W, H);
    }
    if (policy == kBorderPad) {
        int h = H, w = W;
        while (h <= limit && !border_side_ok(h, T, L)) ++h;
        while (w <= limit && !(border_side_ok(w, T, L) && border_area_ok(w, h, L))) ++w;
        if (h > limit || w > limit) return false;
        *Wa = w; *Ha = h;
        return true;
    }
    for (int h = H; h >= 16; --h) {
        if (!border_side_ok(h, T, L)) continue;
        for (int w = W; w >= 16; --w)
            if (border_side_ok(w, T, L) && border_area_ok(w, h, L)) { *Wa = w; *Ha = h; return true; }
    }
    return false;
}

#ifdef __HIPCC__
// One image of one frame: `src` holds H rows of src_pitch elements of eb bytes (the first W of a row are the image), `dst` takes Ha rows
// of Wa.  dst(x, y) = src(x, y) inside the source; outside it the nearest source pixel (replicate) or 0.  Wa <= W / Ha <= H crops.
// in_place: the rows are in dst already (a 2-D copy put them there, src == dst, src_pitch == Wa) and only the margins are written.
struct BorderJob {
    const uint8_t* src;
    uint8_t* dst;
    int W, H, Wa, Ha, src_pitch;
    int eb;                 // bytes per element: 1 (grey, masks), 2 (depth), 3 (colour)
    int replicate, in_place;
    uint32_t first;         // first flat 16-byte unit of the job in the launch (set by launch_frame_border)
    uint32_t units;
};
constexpr int kBorderMaxJobs = 16;     // colour + depth of the eight frames of a batch; colour, depth and two masks of a lone frame
struct BorderStage { int njobs; BorderJob job[kBorderMaxJobs]; };

inline void border_job(BorderJob& j, const void* src, void* dst, int W, int H, int Wa, int Ha, int eb, bool replicate, bool in_place = false) {
    j.src = in_place ? (const uint8_t*)dst : (const uint8_t*)src; j.dst = (uint8_t*)dst;
    j.W = W; j.H = H; j.Wa = Wa; j.Ha = Ha; j.src_pitch = in_place ? Wa : W;
    j.eb = eb; j.replicate = replicate; j.in_place = in_place;
    j.first = 0; j.units = 0;
}
// dst must be 16-byte aligned and Wa * Ha a multiple of 16 (every aligned geometry is); src may start at any byte.
[[nodiscard]] hipError_t launch_frame_border(BorderStage& st, hipStream_t s);
#endif

}  // namespace lm
