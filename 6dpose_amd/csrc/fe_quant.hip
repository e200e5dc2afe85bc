// The quantising side of the front end of Detector::match / addTemplate on gfx950: quantised gradient orientations (LL.cpp:350-505),
// quantised depth normals (LL.cpp:729-819), pyramid steps (LL.cpp:557-581, 857-880) and spread -> response -> linearise
// (LL.cpp:1026-1243) as bytes, written straight into the linear-memory layout the similarity kernels read.
//   upload_normal_lut, clampi, full_add, fast_atan2_deg, quant_angle
//   color_quant_body, grey_quant_body   the colour chain on an RGB and on a one-channel image
//   pyrdown_body, pyrdown_grey_body     cv::pyrDown, 8UC3 and 8UC1
//   k_rgb_to_grey, launch_rgb_to_grey
//   normal_at, normals_median_body, nn_down2_body
//   build_lm_body, build_lm_body4       the byte linear memories (flat + strip-major)
//   k_fe_stage<kCh>                     the one kernel of all of these: a job table, persistent workgroups
//   fe_job_colour, fe_job_normals, fe_job_pyrdown, fe_job_nn_down2, fe_job_build_lm, launch_fe_stage
// The bit planes (k_fe_bits) are fe_bits.hip; what the two share is fe_device.h.
//
// Everything here is HBM/L2-bound byte work on <= a few MB per frame; kernels are one thread per
// output element with coalesced stores.  Parity-critical float steps use the *_rn intrinsics so
// that no FMA contraction or reassociation can occur (the reference is x86-64 SSE2 scalar float,
// OpenCV semantics per SURVEY Appendix A).
#include "launch.h"
#include "fe_device.h"
#include "knobs.h"

namespace lm {

__constant__ uint8_t c_normal_lut[400];   // NORMAL_LUT[.][y][x] (z-independent), normal_lut.i

hipError_t upload_normal_lut(const uint8_t lut400[400]) {
    return hipMemcpyToSymbol(HIP_SYMBOL(c_normal_lut), lut400, 400);
}

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Full adder on 32 bit positions at once (two v_bitop3_b32: parity 0x96, majority 0xE8).  The 3x3 majority vote of the colour chain and the
// 5x5 median of the normals count, per pixel, how many taps of a window satisfy a predicate: with one byte per tap (a bit per predicate) and
// four neighbouring pixels per word, a tree of these adders counts 8 predicates of 4 pixels at once.
static __device__ __forceinline__ void full_add(uint32_t a, uint32_t b, uint32_t c, uint32_t& sum, uint32_t& carry) {
    sum = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
    carry = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
}

// ---- cv::phase(dx, dy, angle, true): OpenCV fastAtan2 polynomial (LL.cpp:423; Appendix A.3) -----
static __device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    const float scale = (float)(180.0 / 3.14159265358979323846);
    const float p1 = __fmul_rn(0.9997878412794807f, scale);
    const float p3 = __fmul_rn(-0.3258083974640975f, scale);
    const float p5 = __fmul_rn(0.1555786518463281f, scale);
    const float p7 = __fmul_rn(-0.04432655554792128f, scale);
    const float eps = 2.220446049250313e-16f;   // (float)DBL_EPSILON
    float ax = fabsf(x), ay = fabsf(y), a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, __fadd_rn(ax, eps));
        c2 = __fmul_rn(c, c);
        a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    } else {
        c = __fdiv_rn(ax, __fadd_rn(ay, eps));
        c2 = __fmul_rn(c, c);
        a = __fsub_rn(90.f,
                      __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c));
    }
    if (x < 0.f) a = __fsub_rn(180.f, a);
    if (y < 0.f) a = __fsub_rn(360.f, a);
    return a;
}
// the 16-bin code of the gradient (bdx, bdy), & 7: saturate_u8(rint(angle * 16 / 360)) & 7 (LL.cpp:423-455), for both colour chains
static __device__ __forceinline__ uint8_t quant_angle(int bdy, int bdx) {
    const float ang = fast_atan2_deg((float)bdy, (float)bdx);
    const float v = rintf(__fmul_rn(ang, (float)(16.0 / 360.0)));   // cvRound: half to even
    const int iv = v < 0.f ? 0 : (v > 255.f ? 255 : (int)v);
    return (uint8_t)(iv & 7);
}

// ---- the colour chain in one launch (LL.cpp:367-504), one 32x16 output tile per workgroup, every intermediate in LDS:
//   cv::GaussianBlur(8UC3, 7x7, sigma 0, BORDER_REPLICATE) (LL.cpp:367; Appendix A.1): separable fixed point, weights
//     [8,28,56,72,56,28,8], out = (sum_ij + 32768) >> 16;
//   Sobel 3x3 (replicate) per channel, strongest channel (first that is >= the other two, LL.cpp:395-412), cv::phase,
//     q16 = interior ? (saturate_u8(rint(angle*16/360)) & 7) : 0 (LL.cpp:368-455);
//   hysteresisGradient's 3x3 majority vote (LL.cpp:457-504).
// Each stage keeps its own border rule by evaluating a stage at the CLAMPED position of the pixel the next stage asks
// for (blur and Sobel replicate the border: smoothed(clamp(p)), not a blur centred outside the image), which makes the
// fused kernel bit-identical to running the stages as separate whole-image passes (the oracle does exactly that).
constexpr int kCTX = 32, kCTY = 16;           // output tile (32 x 32 was measured in round 6: 12 % less halo work, but 29 KB of LDS per workgroup leave a CU 5 of them instead of 7: 52.7 us of kernels per frame against 50.5)
constexpr int kQRowWords = (kCTX + 2 + 3) / 4;   // dwords per row of the vote's / the median's byte planes (34 and 36 bytes -> 9)
static __device__ __forceinline__ void color_quant_body(const int bx, const int by, const uint8_t* __restrict__ rgb, float* __restrict__ mag,
                                                        uint8_t* __restrict__ onehot, int W, int H, float thr_sq) {
    // virtual coordinates: tile origin (x0, y0); halos: rgb 5, blurred 2, quantised 1.
    // The three channels of a pixel travel as ONE LDS word (R | G << 8 | B << 16) and R, B share the multiply-adds of the horizontal
    // pass (7 taps x 255 x 72 <= 65280 fits 16 bits): the stage was bound by its byte-wide LDS reads (21 + 21 + 24 per output pixel;
    // now 7 + 7 + 8).  The integer results are the same.
    __shared__ uint32_t s_rgb[kCTY + 10][kCTX + 10];
    __shared__ uint2 s_tmp[kCTY + 10][kCTX + 4];           // horizontal pass at columns clamp(x0-2 .. x0+TX+1), all halo rows: {R | B << 16, G}
    __shared__ uint32_t s_sm[kCTY + 4][kCTX + 4];           // smoothed at clamp(y0-2 ..), clamp(x0-2 ..), packed like s_rgb
    __shared__ uint32_t s_q4[(kCTY + 2) * kQRowWords];      // ONE-HOT of the 16-bin code & 7 at y0-1 .., x0-1 .. (bin 0 outside the interior), a byte per pixel, rows of kQRowWords dwords
    __shared__ __attribute__((aligned(16))) float s_mag[kCTY][kCTX];
    const int x0 = bx * kCTX, y0 = by * kCTY, tid = threadIdx.x;
    const uint32_t w7[7] = {8, 28, 56, 72, 56, 28, 8};
    for (int i = tid; i < (kCTY + 10) * (kCTX + 10); i += 256) {
        const int ty = i / (kCTX + 10), tx = i - ty * (kCTX + 10);
        const uint8_t* p = rgb + ((size_t)clampi(y0 - 5 + ty, 0, H - 1) * W + clampi(x0 - 5 + tx, 0, W - 1)) * 3;
        s_rgb[ty][tx] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    __syncthreads();
    // horizontal pass: rows = all halo rows (virtual y0-5+ty, already clamped by the load), columns cx = clamp(x0-2+tx)
    for (int i = tid; i < (kCTY + 10) * (kCTX + 4); i += 256) {
        const int ty = i / (kCTX + 4), tx = i - ty * (kCTX + 4);
        const int cx = clampi(x0 - 2 + tx, 0, W - 1) - (x0 - 5);           // tile column of the clamped centre
        uint32_t arb = 0, ag = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const uint32_t px = s_rgb[ty][cx + k - 3];
            arb += w7[k] * (px & 0x00FF00FFu);
            ag += w7[k] * ((px >> 8) & 0xFFu);
        }
        s_tmp[ty][tx] = make_uint2(arb, ag);
    }
    __syncthreads();
    // vertical pass at rows cy = clamp(y0-2+ty)
    for (int i = tid; i < (kCTY + 4) * (kCTX + 4); i += 256) {
        const int ty = i / (kCTX + 4), tx = i - ty * (kCTX + 4);
        const int cy = clampi(y0 - 2 + ty, 0, H - 1) - (y0 - 5);           // tile row of the clamped centre
        uint32_t ar = 0, ag = 0, ab = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const uint2 t = s_tmp[cy + k - 3][tx];
            ar += w7[k] * (t.x & 0xFFFFu); ab += w7[k] * (t.x >> 16); ag += w7[k] * t.y;
        }
        s_sm[ty][tx] = ((ar + 32768u) >> 16) | (((ag + 32768u) >> 16) << 8) | (((ab + 32768u) >> 16) << 16);
    }
    __syncthreads();
    // Sobel + strongest channel + quantisation at (y0-1+ty, x0-1+tx); s_sm index of virtual (vy, vx) = (vy - y0 + 2, vx - x0 + 2)
    for (int i = tid; i < (kCTY + 2) * (kCTX + 2); i += 256) {
        const int ty = i / (kCTX + 2), tx = i - ty * (kCTX + 2);
        const int y = y0 - 1 + ty, x = x0 - 1 + tx;
        uint8_t q = 0;
        if (x >= 0 && y >= 0 && x < W && y < H) {
            const int sy = ty + 1, sx = tx + 1;                             // this pixel in s_sm; its neighbours are the clamped ones by construction
            int dxs[3], dys[3], mags[3];
            {
                // the 3x3 neighbourhood as packed words; R and B ride one 32-bit lane each way (a + 2 b + c <= 1020 fits 16 bits)
                const uint32_t p00 = s_sm[sy - 1][sx - 1], p01 = s_sm[sy - 1][sx], p02 = s_sm[sy - 1][sx + 1];
                const uint32_t p10 = s_sm[sy][sx - 1], p12 = s_sm[sy][sx + 1];
                const uint32_t p20 = s_sm[sy + 1][sx - 1], p21 = s_sm[sy + 1][sx], p22 = s_sm[sy + 1][sx + 1];
                auto rb = [](uint32_t p) { return p & 0x00FF00FFu; };
                auto gg = [](uint32_t p) { return (p >> 8) & 0xFFu; };
                const uint32_t xp_rb = rb(p02) + 2u * rb(p12) + rb(p22), xn_rb = rb(p00) + 2u * rb(p10) + rb(p20);
                const uint32_t yp_rb = rb(p20) + 2u * rb(p21) + rb(p22), yn_rb = rb(p00) + 2u * rb(p01) + rb(p02);
                const int xp_g = (int)(gg(p02) + 2u * gg(p12) + gg(p22)), xn_g = (int)(gg(p00) + 2u * gg(p10) + gg(p20));
                const int yp_g = (int)(gg(p20) + 2u * gg(p21) + gg(p22)), yn_g = (int)(gg(p00) + 2u * gg(p01) + gg(p02));
                dxs[0] = (int)(xp_rb & 0xFFFFu) - (int)(xn_rb & 0xFFFFu); dys[0] = (int)(yp_rb & 0xFFFFu) - (int)(yn_rb & 0xFFFFu);
                dxs[1] = xp_g - xn_g;                                     dys[1] = yp_g - yn_g;
                dxs[2] = (int)(xp_rb >> 16) - (int)(xn_rb >> 16);         dys[2] = (int)(yp_rb >> 16) - (int)(yn_rb >> 16);
#pragma unroll
                for (int c = 0; c < 3; ++c) mags[c] = dxs[c] * dxs[c] + dys[c] * dys[c];
            }
            int bdx, bdy, bmag;
            if (mags[0] >= mags[1] && mags[0] >= mags[2]) { bdx = dxs[0]; bdy = dys[0]; bmag = mags[0]; }
            else if (mags[1] >= mags[0] && mags[1] >= mags[2]) { bdx = dxs[1]; bdy = dys[1]; bmag = mags[1]; }
            else { bdx = dxs[2]; bdy = dys[2]; bmag = mags[2]; }
            if (ty >= 1 && ty <= kCTY && tx >= 1 && tx <= kCTX) s_mag[ty - 1][tx - 1] = (float)bmag;
            if (x > 0 && y > 0 && x < W - 1 && y < H - 1) q = quant_angle(bdy, bdx);
        }
        reinterpret_cast<uint8_t*>(s_q4)[ty * (kQRowWords * 4) + tx] = (uint8_t)(1u << q);
    }
    __syncthreads();
    // hysteresisGradient's vote (LL.cpp:457-504): the orientation that at least 5 of the 9 pixels of the 3x3 window carry (a strict maximum of
    // >= 5 votes of 9 is that orientation; fewer: nothing).  Four pixels per thread: the 9 taps are words of four one-hot bytes (two aligned
    // reads + v_alignbyte per row), a carry-save tree counts all 8 orientations of the 4 pixels at once, count >= 5 <=> b3 | b2 & (b1 | b0).
    // (Was: 9 byte reads + a packed histogram + an 8-way arg-max per pixel, 58 VALU; now ~12.)
    if (tid < kCTY * kCTX / 4) {
        const int ty = tid >> 3, c = tid & 7;
        const int y = y0 + ty, x = x0 + 4 * c;
        if (x < W && y < H) {
            uint32_t sr[3], kr[3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const uint32_t lo = s_q4[(ty + dy) * kQRowWords + c], hi = s_q4[(ty + dy) * kQRowWords + c + 1];
                full_add(lo, __builtin_amdgcn_alignbyte(hi, lo, 1), __builtin_amdgcn_alignbyte(hi, lo, 2), sr[dy], kr[dy]);
            }
            uint32_t b0, k3, u, k4;
            full_add(sr[0], sr[1], sr[2], b0, k3);            // weight 1 done; weight 2: kr[0..2], k3
            full_add(kr[0], kr[1], kr[2], u, k4);
            const uint32_t b1 = u ^ k3, k5 = u & k3;          // weight 4: k4 k5
            const uint32_t b2 = k4 ^ k5, b3 = k4 & k5;
            const uint32_t win = b3 | (b2 & (b1 | b0));
            const size_t o = (size_t)y * W + x;
            const bool yin = y > 0 && y < H - 1;
            uint32_t keep = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float m = s_mag[ty][4 * c + q];
                if (yin && x + q > 0 && x + q < W - 1 && m > thr_sq) keep |= 0xFFu << (8 * q);
                if (mag && x + q < W) mag[o + q] = m;         // (null for the frames of a match: only addTemplate reads the magnitudes, LL.cpp:589-643)
            }
            const uint32_t res = win & keep;
            if (x + 3 < W && ((reinterpret_cast<uintptr_t>(onehot) + o) & 3) == 0) *reinterpret_cast<uint32_t*>(onehot + o) = res;
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x + q < W) onehot[o + q] = (uint8_t)(res >> (8 * q));
            }
        }
    }
}

// ---- the colour chain on a ONE-channel image (a detector with colour_channels = 1: kFeColourGrey) ----
// quantizedOrientations on a frame whose three channels are equal takes channel 0 everywhere (mag1 >= mag2 && mag1 >= mag3, LL.cpp:395-412),
// so this is color_quant_body on the replicated image, byte for byte, with what one channel allows: a byte per pixel in LDS (6.4 KB of
// intermediates against 17.4), the horizontal pass on four pixels per thread from three dwords (two 16-bit sums per multiply-add: 256 x 255
// fits), the vertical pass on two.  The border rule is the same — every stage evaluated at the clamped position — but taken at the other end:
// the tile is LOADED at clamped positions, both blur passes then run on the tile's own (virtual) grid, which makes their taps regular, and
// Sobel picks its neighbours at the clamped index.  smoothed(p) of a pixel p inside the image only ever reads clamped loads, so it is the
// replicate-border blur; virtual positions outside the image hold values nothing reads.
static __device__ __forceinline__ void grey_quant_body(const int bx, const int by, const uint8_t* __restrict__ img, float* __restrict__ mag,
                                                       uint8_t* __restrict__ onehot, int W, int H, float thr_sq) {
    constexpr int kGRow = (kCTX + 10 + 3) / 4;                                       // dwords per row of the loaded tile (42 bytes -> 11)
    __shared__ uint32_t s_g[(kCTY + 10) * kGRow];                                    // pixels at clamp(y0-5 ..), clamp(x0-5 ..), a byte each
    __shared__ __attribute__((aligned(8))) uint16_t s_tmp[kCTY + 10][kCTX + 4];      // horizontal pass at virtual columns x0-2 .. x0+TX+1, all halo rows
    __shared__ __attribute__((aligned(4))) uint8_t s_sm[kCTY + 4][kCTX + 4];         // smoothed at virtual y0-2 .., x0-2 ..
    __shared__ uint32_t s_q4[(kCTY + 2) * kQRowWords];                               // as in color_quant_body
    __shared__ __attribute__((aligned(16))) float s_mag[kCTY][kCTX];
    const int x0 = bx * kCTX, y0 = by * kCTY, tid = threadIdx.x;
    const uint32_t w7[7] = {8, 28, 56, 72, 56, 28, 8};
    for (int i = tid; i < (kCTY + 10) * (kCTX + 10); i += 256) {
        const int ty = i / (kCTX + 10), tx = i - ty * (kCTX + 10);
        reinterpret_cast<uint8_t*>(s_g)[ty * (kGRow * 4) + tx] = img[(size_t)clampi(y0 - 5 + ty, 0, H - 1) * W + clampi(x0 - 5 + tx, 0, W - 1)];
    }
    __syncthreads();
    // horizontal pass: a thread takes four neighbouring columns 4 g .. 4 g + 3 of a row; their taps are bytes 4 g .. 4 g + 9 of the row.
    // word k = bytes k .. k + 3: its even bytes are tap k of columns 0 and 2, its odd bytes tap k of columns 1 and 3.
    if (tid < (kCTY + 10) * ((kCTX + 4) / 4)) {
        const int ty = tid / ((kCTX + 4) / 4), g = tid - ty * ((kCTX + 4) / 4);
        const uint32_t d0 = s_g[ty * kGRow + g], d1 = s_g[ty * kGRow + g + 1], d2 = s_g[ty * kGRow + g + 2];
        const uint32_t wk[7] = {d0, __builtin_amdgcn_alignbyte(d1, d0, 1), __builtin_amdgcn_alignbyte(d1, d0, 2), __builtin_amdgcn_alignbyte(d1, d0, 3),
                                d1, __builtin_amdgcn_alignbyte(d2, d1, 1), __builtin_amdgcn_alignbyte(d2, d1, 2)};
        uint32_t p02 = 0, p13 = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            p02 += w7[k] * (wk[k] & 0x00FF00FFu);
            p13 += w7[k] * ((wk[k] >> 8) & 0x00FF00FFu);
        }
        *reinterpret_cast<uint2*>(&s_tmp[ty][4 * g]) = make_uint2((p02 & 0xFFFFu) | (p13 << 16), (p02 >> 16) | (p13 & 0xFFFF0000u));
    }
    __syncthreads();
    // vertical pass: two neighbouring columns per thread, a dword of two 16-bit sums per tap
    for (int i = tid; i < (kCTY + 4) * ((kCTX + 4) / 2); i += 256) {
        const int ty = i / ((kCTX + 4) / 2), p = i - ty * ((kCTX + 4) / 2);
        uint32_t a0 = 0, a1 = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const uint32_t t = *reinterpret_cast<const uint32_t*>(&s_tmp[ty + k][2 * p]);
            a0 += w7[k] * (t & 0xFFFFu); a1 += w7[k] * (t >> 16);
        }
        *reinterpret_cast<uint16_t*>(&s_sm[ty][2 * p]) = (uint16_t)(((a0 + 32768u) >> 16) | (((a1 + 32768u) >> 16) << 8));
    }
    __syncthreads();
    // Sobel + quantisation at (y0-1+ty, x0-1+tx); s_sm index of virtual (vy, vx) = (vy - y0 + 2, vx - x0 + 2), neighbours at the clamped position
    for (int i = tid; i < (kCTY + 2) * (kCTX + 2); i += 256) {
        const int ty = i / (kCTX + 2), tx = i - ty * (kCTX + 2);
        const int y = y0 - 1 + ty, x = x0 - 1 + tx;
        uint8_t q = 0;
        if (x >= 0 && y >= 0 && x < W && y < H) {
            const int sy = ty + 1, sx = tx + 1;
            const int ym = y > 0 ? sy - 1 : sy, yp = y < H - 1 ? sy + 1 : sy, xm = x > 0 ? sx - 1 : sx, xp = x < W - 1 ? sx + 1 : sx;
            const int p00 = s_sm[ym][xm], p01 = s_sm[ym][sx], p02 = s_sm[ym][xp];
            const int p10 = s_sm[sy][xm], p12 = s_sm[sy][xp];
            const int p20 = s_sm[yp][xm], p21 = s_sm[yp][sx], p22 = s_sm[yp][xp];
            const int bdx = (p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20), bdy = (p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02);
            const int bmag = bdx * bdx + bdy * bdy;
            if (ty >= 1 && ty <= kCTY && tx >= 1 && tx <= kCTX) s_mag[ty - 1][tx - 1] = (float)bmag;
            if (x > 0 && y > 0 && x < W - 1 && y < H - 1) q = quant_angle(bdy, bdx);
        }
        reinterpret_cast<uint8_t*>(s_q4)[ty * (kQRowWords * 4) + tx] = (uint8_t)(1u << q);
    }
    __syncthreads();
    // hysteresisGradient's vote and the stores: color_quant_body's, statement for statement.  Two copies on purpose: as one function over s_q4
    // and s_mag (pointers or array references, with or without __restrict__) both instantiations of k_fe_stage compile to other instructions
    // (4 more each; with LM_DIAG 12 more / 20 fewer and other SGPR spill counts), and the RGB body's are what every RGB detector has run since round 6
    if (tid < kCTY * kCTX / 4) {
        const int ty = tid >> 3, c = tid & 7;
        const int y = y0 + ty, x = x0 + 4 * c;
        if (x < W && y < H) {
            uint32_t sr[3], kr[3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const uint32_t lo = s_q4[(ty + dy) * kQRowWords + c], hi = s_q4[(ty + dy) * kQRowWords + c + 1];
                full_add(lo, __builtin_amdgcn_alignbyte(hi, lo, 1), __builtin_amdgcn_alignbyte(hi, lo, 2), sr[dy], kr[dy]);
            }
            uint32_t b0, k3, u, k4;
            full_add(sr[0], sr[1], sr[2], b0, k3);
            full_add(kr[0], kr[1], kr[2], u, k4);
            const uint32_t b1 = u ^ k3, k5 = u & k3;
            const uint32_t b2 = k4 ^ k5, b3 = k4 & k5;
            const uint32_t win = b3 | (b2 & (b1 | b0));
            const size_t o = (size_t)y * W + x;
            const bool yin = y > 0 && y < H - 1;
            uint32_t keep = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float m = s_mag[ty][4 * c + q];
                if (yin && x + q > 0 && x + q < W - 1 && m > thr_sq) keep |= 0xFFu << (8 * q);
                if (mag && x + q < W) mag[o + q] = m;
            }
            const uint32_t res = win & keep;
            if (x + 3 < W && ((reinterpret_cast<uintptr_t>(onehot) + o) & 3) == 0) *reinterpret_cast<uint32_t*>(onehot + o) = res;
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x + q < W) onehot[o + q] = (uint8_t)(res >> (8 * q));
            }
        }
    }
}

// ---- cv::pyrDown 8UC3 (LL.cpp:566; Appendix A.6): 5x5 [1 4 6 4 1], REFLECT_101, (sum+128)>>8 ----
static __device__ __forceinline__ int reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

static __device__ __forceinline__ void pyrdown_body(const int bx, const int by, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H,
                                                    int Wo, int Ho) {
    int i = bx * 256 + threadIdx.x, y = by;   // i over Wo*3
    if (i >= Wo * 3) return;
    int x = i / 3, c = i - x * 3;
    const int w[5] = {1, 4, 6, 4, 1};
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* row = src + (size_t)reflect101(2 * y + j - 2, H) * W * 3;
        int rs = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) rs += w[k] * row[reflect101(2 * x + k - 2, W) * 3 + c];
        s += w[j] * rs;
    }
    dst[(size_t)y * Wo * 3 + i] = (uint8_t)((s + 128) >> 8);
}

// cv::pyrDown 8UC1 (kFePyrDownGrey): a thread per output pixel, where pyrdown_body takes one per output byte; the two share no statement
static __device__ __forceinline__ void pyrdown_grey_body(const int bx, const int by, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H,
                                                         int Wo, int Ho) {
    const int x = bx * 256 + threadIdx.x, y = by;
    if (x >= Wo) return;
    const int w[5] = {1, 4, 6, 4, 1};
    int cx[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) cx[k] = reflect101(2 * x + k - 2, W);
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* row = src + (size_t)reflect101(2 * y + j - 2, H) * W;
        int rs = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) rs += w[k] * row[cx[k]];
        s += w[j] * rs;
    }
    dst[(size_t)y * Wo + x] = (uint8_t)((s + 128) >> 8);
}

// (4899 R + 9617 G + 1868 B + 8192) >> 14: the 8-bit fixed point of OpenCV's RGB2GRAY.  UNPINNED: stated from OpenCV's documentation of the
// conversion, not checked against an OpenCV build (none here); rgb_to_grey_ref in lm_abi.py is the same formula in numpy and the tests hold the two together.
__global__ void __launch_bounds__(256) k_rgb_to_grey(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ grey, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = rgb + 3 * i;
    grey[i] = (uint8_t)((4899u * p[0] + 9617u * p[1] + 1868u * p[2] + 8192u) >> 14);
}
hipError_t launch_rgb_to_grey(const uint8_t* rgb, uint8_t* grey, size_t pixels, hipStream_t s) {
    return pixels ? lm_launch(k_rgb_to_grey, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, rgb, grey, pixels) : hipSuccess;
}

// ---- quantizedNormals (LL.cpp:729-817; Appendix A.7) + cv::medianBlur(5) (LL.cpp:818), replicate border ----------
// One launch: the raw normals of a 32x16 tile (+2 halo, evaluated at the clamped positions medianBlur's replicate
// border asks for) live in LDS.  Values are 0 or one-hot -> 9 ranks; the median is the 13th smallest of 25, found with
// packed 5-bit counters in a 64-bit word.
static __device__ __forceinline__ uint8_t normal_at(const uint16_t* __restrict__ depth, int x, int y, int W, int H, int dist_thr, int diff_thr) {
    const int r = 5;
    uint8_t res = 0;
    if (x >= r && y >= r && x < W - r - 1 && y < H - r - 1) {
        const uint16_t* p = depth + (size_t)y * W + x;
        long long d = p[0];
        if (d < dist_thr) {
            const int oi[8] = {-r, 0, r, -r, r, -r, 0, r};
            const int oj[8] = {-r, -r, -r, 0, 0, r, r, r};
            float nx, ny, nz;
            if (diff_thr <= 150) {
                // the reference's `long` arithmetic (LL.cpp:701-819) in 32 bits: |delta| < diff_thr on every tap that counts, so
                // |b| <= 40 diff_thr, |ddx|, |ddy| <= 12000 diff_thr, 1150 |ddx| <= 1.38e7 diff_thr < 2^31 and det * d <= 22500 * 65535
                // < 2^31 — the same integers, a third of the instructions (64-bit multiplies are emulated)
                int A0 = 0, A1 = 0, A3 = 0, b0 = 0, b1 = 0;
                const int di = (int)d;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int delta = (int)p[oj[k] * W + oi[k]] - di;
                    const int ad = delta < 0 ? -delta : delta;
                    if (ad < diff_thr) {
                        A0 += oi[k] * oi[k]; A1 += oi[k] * oj[k]; A3 += oj[k] * oj[k];
                        b0 += oi[k] * delta; b1 += oj[k] * delta;
                    }
                }
                const int det = A0 * A3 - A1 * A1;
                const int ddx = A3 * b0 - A1 * b1;
                const int ddy = -A1 * b0 + A0 * b1;
                nx = (float)(1150 * ddx); ny = (float)(1150 * ddy); nz = (float)(-det * di);
            } else {
                long long A0 = 0, A1 = 0, A3 = 0, b0 = 0, b1 = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    long long delta = (long long)p[oj[k] * W + oi[k]] - d;
                    long long ad = delta < 0 ? -delta : delta;
                    long long f = ad < diff_thr ? 1 : 0;
                    long long fi = f * oi[k], fj = f * oj[k];
                    A0 += fi * oi[k]; A1 += fi * oj[k]; A3 += fj * oj[k];
                    b0 += fi * delta; b1 += fj * delta;
                }
                long long det = A0 * A3 - A1 * A1;
                long long ddx = A3 * b0 - A1 * b1;
                long long ddy = -A1 * b0 + A0 * b1;
                nx = (float)(1150 * ddx); ny = (float)(1150 * ddy); nz = (float)(-det * d);
            }
            float ss = __fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz));
            float sq = __fsqrt_rn(ss);
            if (sq > 0.f) {
                float inv = __fdiv_rn(1.0f, sq);
                nx = __fmul_rn(nx, inv); ny = __fmul_rn(ny, inv); nz = __fmul_rn(nz, inv);
                int v1 = (int)__fadd_rn(__fmul_rn(nx, 10.f), 10.f);
                int v2 = (int)__fadd_rn(__fmul_rn(ny, 10.f), 10.f);
                // v3 = (int)(nz*20+20) only selects the (z-independent) table plane; an index of 20 in
                // x or y continues into the next row exactly as the reference's flat memory read does.
                int flat = (v2 * 20 + v1) % 400;
                if (flat < 0) flat += 400;
                res = c_normal_lut[flat];
            }
        }
    }
    return res;
}

static __device__ __forceinline__ void normals_median_body(const int bx, const int by, const uint16_t* __restrict__ depth, uint8_t* __restrict__ raw,
                                                           uint8_t* __restrict__ med, int W, int H, int dist_thr, int diff_thr) {
    __shared__ uint32_t s_m[(kCTY + 4) * kQRowWords];        // a byte per pixel of the tile + 2: bit k = (rank of the raw normal <= k), rank 0 = none, k + 1 = 1 << k
    const int x0 = bx * kCTX, y0 = by * kCTY, tid = threadIdx.x;
    for (int i = tid; i < (kCTY + 4) * (kCTX + 4); i += 256) {
        const int ty = i / (kCTX + 4), tx = i - ty * (kCTX + 4);
        const int y = clampi(y0 - 2 + ty, 0, H - 1), x = clampi(x0 - 2 + tx, 0, W - 1);
        const uint8_t v = normal_at(depth, x, y, W, H, dist_thr, diff_thr);
        reinterpret_cast<uint8_t*>(s_m)[ty * (kQRowWords * 4) + tx] = (uint8_t)(0xFFu << (32 - __clz((int)v)));   // (__clz(0) = 32)
        if (ty >= 2 && ty < kCTY + 2 && tx >= 2 && tx < kCTX + 2 && y0 - 2 + ty < H && x0 - 2 + tx < W) raw[(size_t)y * W + x] = v;
    }
    __syncthreads();
    // cv::medianBlur(5) of values that are 0 or one-hot = the 13th smallest of 25 ranks: median rank <= k <=> at least 13 taps have rank <= k.
    // Four pixels per thread; a tap word holds the 8 predicates "rank <= k" of 4 neighbouring pixels, a carry-save tree (20 full + 2 half
    // adders) counts them over the 25 taps, count >= 13 <=> b4 | b3 & b2 & (b1 | b0).  The predicates of a pixel are monotone in k, so its byte
    // of the result is 0xFF << rank and the value 1 << (rank - 1) (0 for rank 0) is its lowest set bit (of the byte | 0x100) >> 1.
    // (Was: 25 byte reads into packed 5-bit counters of a 64-bit word + a 9-step scan per pixel, 251 VALU; now ~26.)
    if (tid < kCTY * kCTX / 4) {
        const int ty = tid >> 3, c = tid & 7;
        const int y = y0 + ty, x = x0 + 4 * c;
        if (x < W && y < H) {
            // a row at a time (five taps -> a 3-bit count: 2 full + 1 half adder), added into the bit-sliced total by a ripple adder: a few more
            // operations than one tree over the 25 taps (62 against 44) but a dozen live registers instead of 30 — the tree cost k_fe_stage a wave of occupancy
            uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0;
#pragma unroll
            for (int dy = 0; dy < 5; ++dy) {
                const uint32_t lo = s_m[(ty + dy) * kQRowWords + c], hi = s_m[(ty + dy) * kQRowWords + c + 1];
                uint32_t sa, ka, r0, kb;
                full_add(lo, __builtin_amdgcn_alignbyte(hi, lo, 1), __builtin_amdgcn_alignbyte(hi, lo, 2), sa, ka);
                full_add(sa, __builtin_amdgcn_alignbyte(hi, lo, 3), hi, r0, kb);
                const uint32_t r1 = ka ^ kb, r2 = ka & kb;
                if (dy == 0) { b0 = r0; b1 = r1; b2 = r2; }
                else {
                    const uint32_t k0 = b0 & r0; b0 ^= r0;
                    uint32_t k1, k2;
                    full_add(b1, r1, k0, b1, k1);
                    full_add(b2, r2, k1, b2, k2);
                    const uint32_t k3 = b3 & k2; b3 ^= k2;
                    b4 ^= k3;
                }
            }
            const uint32_t ge = b4 | (b3 & b2 & (b1 | b0));
            uint32_t out = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t B = ((ge >> (8 * q)) & 0xFFu) | 0x100u;
                out |= ((B & (0u - B)) >> 1) << (8 * q);
            }
            const size_t o = (size_t)y * W + x;
            if (x + 3 < W && ((reinterpret_cast<uintptr_t>(med) + o) & 3) == 0) *reinterpret_cast<uint32_t*>(med + o) = out;
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x + q < W) med[o + q] = (uint8_t)(out >> (8 * q));
            }
        }
    }
}

// cv::resize(INTER_NEAREST) to (cols/2, rows/2) (LL.cpp:576, 867, 877) = pixel (2y, 2x)
static __device__ __forceinline__ void nn_down2_body(const int bx, const int by, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int Wo) {
    int x = bx * 256 + threadIdx.x, y = by;
    if (x >= Wo) return;
    dst[(size_t)y * Wo + x] = src[(size_t)(2 * y) * W + 2 * x];
}

// ---- spread (LL.cpp:1094-1109) fused with computeResponseMaps (LL.cpp:1134-1203, active SIMILARITY_LUT
// :1121 in closed form) and linearize (LL.cpp:1215-1243), both modalities of a level in ONE launch ------
// One thread per linear-memory position (phase, decimated index) and modality (blockIdx.z): OR the T x T
// quantised pixels below / right of it (zero beyond the edges; mask applied as quantize() does), derive the
// 8 responses (4 / 1 / 0), store to LM[label][phase][idx] — consecutive lanes write consecutive bytes of
// each label's plane.  Levels below the top also get the "strip" copy the refinement kernel gathers from:
// every plane cut into 16-column strips stored strip-major ([strip][row][16 B]), so that a 16x16 window
// touches 2 strips x 256 contiguous bytes instead of 16 rows x 1 cache line.  (The frame is a few hundred
// KB: the T*T byte reads per thread hit L1/L2; what counts here is one launch instead of four.)
// the response bytes of label `ori` for the spread bytes of v, any table: r[d] = the sum of r[k] - r[k + 1] over k >= d (non-increasing, r[5] = 0)
struct RespBytes {
    uint32_t m[5], w[5];
    __device__ __forceinline__ RespBytes(uint32_t v, uint32_t resp) {
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) {
            m[k] = k == 0 ? v : m[k - 1] | rot_bytes(v, k) | rot_bytes(v, 8u - k);
            w[k] = ((resp >> (4 * k)) & 15u) - (k < 4 ? (resp >> (4 * k + 4)) & 15u : 0u);
        }
    }
    __device__ __forceinline__ uint32_t at(int ori) const {
        uint32_t r = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) r += w[k] * ((m[k] >> ori) & 0x01010101u);
        return r;
    }
};

static __device__ __forceinline__ void build_lm_body(const int bx, const int by, const LmJob& J, int W, int H, int T, int Wd, int Hd, int NS, uint32_t m_wd,
                                                     uint32_t m_t, uint32_t resp) {
    int idx = bx * 256 + threadIdx.x;                    // decimated raster index
    int phase = by;                                      // r_start*T + c_start
    int npos = Wd * Hd;
    if (idx >= npos) return;
    int ry = (int)fast_div((uint32_t)idx, m_wd, (uint32_t)Wd), rx = idx - ry * Wd;
    int rs = (int)fast_div((uint32_t)phase, m_t, (uint32_t)T), cs = phase - rs * T;
    int y = ry * T + rs, x = rx * T + cs;
    const uint32_t v = spread_or(J, x, y, W, H, T);
    uint32_t adj = ((v << 1) | (v >> 7) | (v >> 1) | (v << 7)) & 0xFFu;
    size_t plane = (size_t)T * T * npos;
    uint8_t* o = J.lm + (size_t)phase * npos + idx;
    const size_t splane1 = (size_t)NS * Hd * 16;             // one (label, phase) plane in strip form
    uint8_t* so = J.strips ? J.strips + (size_t)phase * splane1 + ((size_t)(rx >> 4) * Hd + ry) * 16 + (rx & 15) : nullptr;
    if (resp != kRespDefault) {                              // wave-uniform: another table than 4 1 0 0 0
        const RespBytes rb(v, resp);
#pragma unroll
        for (int ori = 0; ori < 8; ++ori) {
            const uint8_t r = (uint8_t)rb.at(ori);
            o[plane * ori] = r;
            if (so) so[splane1 * T * T * ori] = r;
        }
        return;
    }
#pragma unroll
    for (int ori = 0; ori < 8; ++ori) {
        uint8_t r = ((v >> ori) & 1u) ? 4 : (((adj >> ori) & 1u) ? 1 : 0);
        o[plane * ori] = r;
        if (so) so[splane1 * T * T * ori] = r;
    }
}

// The same with dword stores (Wd % 4 == 0: the four positions of a lane quad share a row and a strip): every lane still ORs its own
// T x T pixels, then the quad exchanges the four OR bytes and lane k of the quad stores labels 2k and 2k + 1 for all four positions —
// one dword each to the flat plane and to the strip plane, 4 stores per lane instead of 16 byte stores (the launch is bound by the
// number of store instructions: 44 MB per 4-frame batch took 48 us = 0.9 TB/s).
static __device__ __forceinline__ void build_lm_body4(const int bx, const int by, const LmJob& J, int W, int H, int T, int Wd, int Hd, int NS, uint32_t m_wd,
                                                      uint32_t m_t, uint32_t resp) {
    const int idx = bx * 256 + (int)threadIdx.x;         // decimated raster index
    const int phase = by;
    const int npos = Wd * Hd;
    if (idx >= npos) return;                             // whole quads: npos is a multiple of 4
    const int ry = (int)fast_div((uint32_t)idx, m_wd, (uint32_t)Wd), rx = idx - ry * Wd;
    const int rs = (int)fast_div((uint32_t)phase, m_t, (uint32_t)T), cs = phase - rs * T;
    const int y = ry * T + rs, x = rx * T + cs;
    const uint32_t v = spread_or(J, x, y, W, H, T);
    const int lane = (int)threadIdx.x & 63, k4 = lane & 3, q0 = lane & ~3;
    uint32_t vq[4], adj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        vq[k] = (uint32_t)__shfl((int)v, q0 + k, 64);
        adj[k] = ((vq[k] << 1) | (vq[k] >> 7) | (vq[k] >> 1) | (vq[k] << 7)) & 0xFFu;
    }
    const int idx0 = idx - k4, rx0 = rx - k4;            // first position of the quad
    const size_t plane = (size_t)T * T * npos;
    const size_t splane1 = (size_t)NS * Hd * 16;
    uint8_t* o = J.lm + (size_t)phase * npos + idx0;
    uint8_t* so = J.strips ? J.strips + (size_t)phase * splane1 + ((size_t)(rx0 >> 4) * Hd + ry) * 16 + (rx0 & 15) : nullptr;
    if (resp != kRespDefault) {                              // wave-uniform: another table than 4 1 0 0 0
        const RespBytes rb(vq[0] | (vq[1] << 8) | (vq[2] << 16) | (vq[3] << 24), resp);
#pragma unroll
        for (int li = 0; li < 2; ++li) {
            const int ori = 2 * k4 + li;
            const uint32_t packed = rb.at(ori);
            *reinterpret_cast<uint32_t*>(o + plane * ori) = packed;
            if (so) *reinterpret_cast<uint32_t*>(so + splane1 * T * T * ori) = packed;
        }
        return;
    }
#pragma unroll
    for (int li = 0; li < 2; ++li) {
        const int ori = 2 * k4 + li;
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t r = ((vq[k] >> ori) & 1u) ? 4u : (((adj[k] >> ori) & 1u) ? 1u : 0u);
            packed |= r << (8 * k);
        }
        *reinterpret_cast<uint32_t*>(o + plane * ori) = packed;
        if (so) *reinterpret_cast<uint32_t*>(so + splane1 * T * T * ori) = packed;
    }
}

// ---- several independent front-end jobs in ONE launch ---------------------------------------------------------------------
// The seven jobs of a frame are small (5-17 us as kernels of their own, as they were in round 1) and dependent kernels on a queue
// start ~7 us apart, so the front end is mostly launch latency.  The jobs that do not depend on each other share a launch: stage k = {colour chain of level k,
// normals + median (k = 0) or nearest-neighbour normals of level k, pyrDown to level k + 1}; the last launch builds the linear
// memories of every level.  A job is a range of the flat block index; the *_body functions above are the jobs, and k_fe_stage is their only kernel.
// The workgroups are persistent: a tile takes a workgroup ~1.5 us, and the dispatcher hands an XCD a new workgroup only every
// ~30 ns — with one workgroup per tile (10.8k for the first stage of four VGA frames) a CU held 1.3 workgroups on average and the
// stage took as long as the dispatcher needed (42 us; profiles/r03_pmc.txt: 5 waves per CU).  A few workgroups per CU walk the
// tiles instead (flat index + k * grid).
// kCh = the colour image's channels: the instantiation for 3 holds the RGB colour chain and pyrDown, the one for 1 the grey ones (a detector launches
// one of the two: the bodies' __shared__ arrays add up per kernel, and with both chains inside neither would keep kFeWaves workgroups on a CU).
template <int kCh>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kFeWaves, kFeWaves)))   // kFeWaves persistent workgroups per CU (knobs: fe_wgs_per_cu) = as many waves per SIMD
k_fe_stage(FeStage st, int total) {
    for (int blk = (int)blockIdx.x; blk < total; blk += (int)gridDim.x) {
        int j = 0;
        while (j + 1 < st.njobs && blk >= st.job[j + 1].first) ++j;
        const FeJob& J = st.job[j];
        const int local = blk - J.first;
        const int bz = (int)fast_div((uint32_t)local, J.m_gxgy, (uint32_t)(J.gx * J.gy)), rem = local - bz * J.gx * J.gy;
        const int by = (int)fast_div((uint32_t)rem, J.m_gx, (uint32_t)J.gx), bx = rem - by * J.gx;
        switch (J.kind) {
            case kCh == 3 ? kFeColour : kFeColourGrey:           // (the other instantiation's kinds fall to the default: nothing)
                if (kCh == 3) color_quant_body(bx, by, (const uint8_t*)J.in, (float*)J.out0, (uint8_t*)J.out1, J.W, J.H, J.f);
                else grey_quant_body(bx, by, (const uint8_t*)J.in, (float*)J.out0, (uint8_t*)J.out1, J.W, J.H, J.f);
                break;
            case kFeNormals: normals_median_body(bx, by, (const uint16_t*)J.in, (uint8_t*)J.out0, (uint8_t*)J.out1, J.W, J.H, J.a, J.b); break;
            case kCh == 3 ? kFePyrDown : kFePyrDownGrey:
                if (kCh == 3) pyrdown_body(bx, by, (const uint8_t*)J.in, (uint8_t*)J.out0, J.W, J.H, J.a, J.b);
                else pyrdown_grey_body(bx, by, (const uint8_t*)J.in, (uint8_t*)J.out0, J.W, J.H, J.a, J.b);
                break;
            case kFeNnDown: nn_down2_body(bx, by, (const uint8_t*)J.in, (uint8_t*)J.out0, J.W, J.a); break;
            case kFeBuildLm:
                if ((J.Wd & 3) == 0) build_lm_body4(bx, by, J.lm[bz], J.W, J.H, J.a, J.Wd, J.Hd, (J.Wd + 15) >> 4, J.m_wd, J.m_t, st.resp);
                else build_lm_body(bx, by, J.lm[bz], J.W, J.H, J.a, J.Wd, J.Hd, (J.Wd + 15) >> 4, J.m_wd, J.m_t, st.resp);
                break;
            default: break;
        }
        if (blk + (int)gridDim.x < total) __syncthreads();      // the next tile reuses the bodies' LDS
    }
}

void fe_job_colour(FeJob& j, const uint8_t* rgb, float* mag, uint8_t* onehot, int W, int H, float thr_sq, int channels) {
    j = FeJob{}; j.kind = channels == 1 ? kFeColourGrey : kFeColour; j.gx = (W + kCTX - 1) / kCTX; j.gy = (H + kCTY - 1) / kCTY; j.gz = 1;
    j.in = rgb; j.out0 = mag; j.out1 = onehot; j.W = W; j.H = H; j.f = thr_sq;
}
void fe_job_normals(FeJob& j, const uint16_t* depth, uint8_t* raw, uint8_t* med, int W, int H, int dist_thr, int diff_thr) {
    j = FeJob{}; j.kind = kFeNormals; j.gx = (W + kCTX - 1) / kCTX; j.gy = (H + kCTY - 1) / kCTY; j.gz = 1;
    j.in = depth; j.out0 = raw; j.out1 = med; j.W = W; j.H = H; j.a = dist_thr; j.b = diff_thr;
}
void fe_job_pyrdown(FeJob& j, const uint8_t* src, uint8_t* dst, int W, int H, int channels) {
    j = FeJob{}; j.kind = channels == 1 ? kFePyrDownGrey : kFePyrDown; j.a = W / 2; j.b = H / 2; j.gx = (j.a * channels + 255) / 256; j.gy = j.b; j.gz = 1;
    j.in = src; j.out0 = dst; j.W = W; j.H = H;
}
void fe_job_nn_down2(FeJob& j, const uint8_t* src, uint8_t* dst, int W, int H) {
    j = FeJob{}; j.kind = kFeNnDown; j.a = W / 2; j.gx = (j.a + 255) / 256; j.gy = H / 2; j.gz = 1;
    j.in = src; j.out0 = dst; j.W = W; j.H = H;
}
// The writers of response memories run over the modalities [m0, m0 + nm) of the arrays they are given (indexed by kind: [0] colour, [1] normals):
// the job's blocks are gz = nm slices, slice z serves j.lm[z] = modality m0 + z.  A detector with one modality therefore launches half the blocks
// and its kernels never see the other modality's pointers.
void fe_job_build_lm(FeJob& j, const uint8_t* const quant[2], const uint8_t* const mask[2], uint8_t* const lm[2], uint8_t* const strips[2],
                     int W, int H, int T, int m0, int nm) {
    fe_job_lm_grid(j, kFeBuildLm, W, H, T, nm);
    j.gx = (j.Wd * j.Hd + 255) / 256;
    for (int z = 0; z < nm; ++z) j.lm[z] = LmJob{quant[m0 + z], mask[m0 + z], lm[m0 + z], strips[m0 + z]};
}
hipError_t launch_fe_stage(FeStage& st, hipStream_t s) {
    const int total = fe_prepare(st);
    if (total <= 0) return hipSuccess;
    const int per_cu = knobs().fe_wgs_per_cu;
    const int grid = per_cu > 0 ? std::min(total, fe_cus() * per_cu) : total;
    bool grey = false;                                               // the grey kinds come from a detector with colour_channels = 1, which never adds the RGB ones
    for (int i = 0; i < st.njobs; ++i) grey = grey || st.job[i].kind == kFeColourGrey || st.job[i].kind == kFePyrDownGrey;
    return lm_launch(grey ? k_fe_stage<1> : k_fe_stage<3>, dim3(grid), dim3(256), 0, s, st, total);
}

}  // namespace lm
