// k_frame_border: the uploaded sources of a frame (rows of W elements) -> the frame buffers of the aligned geometry (rows of Wa), padded at
// the right and bottom (edge replication for colour / grey, zeros for depth and masks) or cropped there.  One launch serves every image
// of every frame of a batch (BorderStage, frame_border.h).
//
// The destination is walked in 16-byte units, one per thread, each stored with one dwordx4: a frame buffer starts 16-byte aligned and
// Wa * Ha is a multiple of 16, so its bytes are a whole number of units whatever Wa is.  A unit that lies inside one source row (all but
// one or two per row) is 16 consecutive source bytes; they start at any byte offset (W odd, colour rows of 3 W bytes, the depth image
// behind a colour image of odd size), so they are fetched as the aligned dwords that cover them and shifted into place.  The other units
// — across a row end, in the margins — are put together byte by byte.
#include "launch.h"
#include "frame_border.h"

namespace lm {

__device__ __forceinline__ uint32_t border_byte(const BorderJob& j, int x, int y, int c) {
    if (j.replicate) { x = min(x, j.W - 1); y = min(y, j.H - 1); }
    else if (x >= j.W || y >= j.H) return 0u;
    return j.src[((size_t)y * j.src_pitch + x) * j.eb + c];
}

__global__ __launch_bounds__(256) void k_frame_border(const BorderStage st, uint32_t total) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    int ji = 0;
    while (ji + 1 < st.njobs && u >= st.job[ji + 1].first) ++ji;
    const BorderJob& j = st.job[ji];
    const uint32_t o = (u - j.first) * 16u;                  // byte offset of the unit in dst (< Wa * Ha * eb <= 3 * 2^28)
    const uint32_t row_bytes = (uint32_t)j.Wa * j.eb;
    const uint32_t inner_bytes = (uint32_t)min(j.W, j.Wa) * j.eb;
    int y = (int)(o / row_bytes);
    const uint32_t xb = o - (uint32_t)y * row_bytes;
    uint32_t out[4];
    if (y < j.H && xb + 16u <= inner_bytes) {                // 16 consecutive source bytes
        if (j.in_place) return;                              // ... which a 2-D copy has put there
        const uint8_t* sp = j.src + (size_t)y * j.src_pitch * j.eb + xb;
        const uint32_t sh = (uint32_t)((uintptr_t)sp & 3u);
        const uint32_t* ap = reinterpret_cast<const uint32_t*>(sp - sh);
        uint32_t d[5];
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = ap[k];
        d[4] = sh ? ap[4] : 0u;                              // (sh != 0: the fifth dword holds the unit's last byte, so it lies in the source)
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> (8u * sh));
    } else {
        int x = (int)(j.eb == 3 ? xb / 3u : xb >> (j.eb - 1));
        int c = (int)(xb - (uint32_t)x * j.eb);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                v |= border_byte(j, x, y, c) << (8 * b);
                if (++c == j.eb) { c = 0; if (++x == j.Wa) { x = 0; ++y; } }
            }
            out[k] = v;
        }
    }
    *reinterpret_cast<uint4*>(j.dst + o) = make_uint4(out[0], out[1], out[2], out[3]);
}

hipError_t launch_frame_border(BorderStage& st, hipStream_t s) {
    uint32_t total = 0;
    for (int i = 0; i < st.njobs; ++i) {
        BorderJob& j = st.job[i];
        j.first = total;
        j.units = (uint32_t)(((size_t)j.Wa * j.Ha * j.eb) / 16);
        total += j.units;
    }
    if (!total) return hipSuccess;
    return lm_launch(k_frame_border, dim3((total + 255u) / 256u), dim3(256), 0, s, st, total);
}

}  // namespace lm
