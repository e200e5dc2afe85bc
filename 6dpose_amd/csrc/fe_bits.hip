// The bit-plane side of the front end on gfx950: spread -> response -> linearise (LL.cpp:1026-1243, the live SIMILARITY_LUT :1121) written
// as the two bit planes per label that the bit-plane matching kernels read (match_bits.hip), when nothing reads
// the byte planes of fe_quant.hip.
//   within, resp_planes                                   the response table as two bit planes
//   bits_rows_body, bits_rows_block_body<kT>              strip records of a level below the top: per thread, and from pixel tiles
//   top_bits_body, top_bits_aligned_body, top_bits_tile_body<kT> (tile_spread, transpose8x8)   the top level's pair stream
//   fe_bits_rows, fe_top_tile_fits, fe_rows_tile_fits, fe_rows_block_rows                      which writer a geometry allows
//   k_fe_bits                                             the one kernel of all of these: k_fe_stage's job table and persistent walk
//   fe_bits_rows_possible, fe_job_bits_rows, fe_top_bits_kind, fe_job_top_bits, launch_fe_bits
// What it shares with fe_quant.hip is fe_device.h.
#include "launch.h"
#include "fe_device.h"
#include "knobs.h"

namespace lm {

// ---- the response table (lm_kernels.h, resp_pack).  Every byte of a word is a spread byte (a lone one: the upper bytes zero). ----
// bit `ori` of a byte: some orientation bit of the spread byte lies at cyclic distance <= k from ori
static __device__ __forceinline__ uint32_t within(uint32_t v, uint32_t k) {
    uint32_t m = v;
    for (uint32_t d = 1; d <= k; ++d) m |= rot_bytes(v, d) | rot_bytes(v, 8u - d);
    return m;
}
// the two bit planes of a table with at most two distinct non-zero values: hi = "the response is 4", lo = "it is the second value".
// The default table (4 1 0 0 0) keeps the two rotations it always took.
static __device__ __forceinline__ void resp_planes(uint32_t v, uint32_t resp, uint32_t& hi, uint32_t& lo) {
    if (resp == kRespDefault) {                                         // wave-uniform
        hi = v;
        lo = (((v << 1) & 0xFEFEFEFEu) | ((v >> 7) & 0x01010101u) | ((v >> 1) & 0x7F7F7F7Fu) | ((v << 7) & 0x80808080u)) & ~v;
    } else {
        hi = within(v, (resp >> 20) & 7u);
        lo = within(v, (resp >> 24) & 7u) & ~hi;
    }
}

// ---- the bit planes written directly -------------------------------------------------------------------------------
// When nothing reads the byte planes of a level (bit-plane kernels for both passes, every window inside its plane) the linear-memory
// stage does not write them at all: 8 response bytes per position and encoding (flat + strip-major: 9.8 MB per VGA frame at level 0)
// become 2 bits per position and label (2.5 MB), and k_pack_bits / k_pack_top disappear from the batch.
//
// Strip records of a level below the top (match_bits.hip: per plane row and 16-column strip 64 bits, cell c of [16 s, 16 s + 32) at bits 2c =
// "response is 1" and 2c + 1 = "response is 4").  A workgroup takes R rows of one (modality, phase): every thread ORs the T x T
// pixels of a few cells (spread) and leaves {neighbour bits & ~own bits | own bits << 8} per cell in LDS — response 4 iff the label's own
// bit is set, 1 iff only a neighbouring label's is (LL.cpp:1121) —; then one thread per (label, row, strip) gathers the label's two bits of
// its 32 cells into a record.  Rows fastest in the thread order: the records of a strip's R rows are R x 8 contiguous bytes.
constexpr int kBitsCells = 1152;              // 16-bit cell words of a workgroup's rows in LDS: R x (16 NS + 16) <= this (VGA level 0: 6 x 176)
static __host__ __device__ inline int fe_bits_rows(int Wd) { const int wp = ((Wd + 15) / 16) * 16 + 16; const int r = kBitsCells / wp; return r < 8 ? r : 8; }

static __device__ __forceinline__ void bits_rows_body(const int bx, const int by, const LmJob& J, int W, int H, int T, int Wd, int Hd, int NS, uint32_t m_wd,
                                                      uint32_t m_t, uint16_t* __restrict__ s_cells /* kBitsCells */, uint32_t resp) {
    const int Wp = NS * 16 + 16, R = fe_bits_rows(Wd);
    const int phase = by, ry0 = bx * R;
    const int rows = Hd - ry0 < R ? Hd - ry0 : R;
    const int rs = (int)fast_div((uint32_t)phase, m_t, (uint32_t)T), cs = phase - rs * T;
    // every thread's cells (<= kBitsCells / 256, rounded up) at once: their pixel loads are all in flight together
    constexpr int kPer = (kBitsCells + 255) / 256;
    const float inv_wp = 1.0f / (float)Wp;
    uint32_t w[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        const int r = (int)(((float)i + 0.5f) * inv_wp), rx = i - r * Wp;      // exact: i < 2048, Wp >= 32
        w[k] = 0;
        if (i < rows * Wp && rx < Wd) {
            const uint32_t v = spread_or(J, rx * T + cs, (ry0 + r) * T + rs, W, H, T);
            uint32_t hi, lo;
            resp_planes(v, resp, hi, lo);
            w[k] = lo | (hi << 8);
        }
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        if (i < rows * Wp) s_cells[i] = (uint16_t)w[k];
    }
    __syncthreads();
    const size_t splane1 = (size_t)NS * Hd * 8;                           // one (label, phase) plane of records
    uint8_t* out = J.lm + (size_t)phase * splane1;
    const float inv_rows = 1.0f / (float)rows, inv_ns = 1.0f / (float)NS;
    for (int i = (int)threadIdx.x; i < 8 * rows * NS; i += 256) {
        const int q = (int)(((float)i + 0.5f) * inv_rows), r = i - q * rows;   // (small integers: the float quotients are exact)
        const int label = (int)(((float)q + 0.5f) * inv_ns), st = q - label * NS;
        const uint32_t* cw = reinterpret_cast<const uint32_t*>(s_cells + r * Wp + 16 * st);     // 32 cells = 16 dwords of two cells each
        uint32_t lo = 0, hi = 0;
#pragma unroll 2
        for (int k = 0; k < 8; ++k) {
            // bits label and 8 + label of two cells -> {is 1, is 4, is 1, is 4}
            lo |= (((((cw[k] >> label) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (4 * k);
            hi |= (((((cw[8 + k] >> label) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (4 * k);
        }
        *reinterpret_cast<uint2*>(out + (size_t)label * T * T * splane1 + ((size_t)st * Hd + ry0 + r) * 8) = make_uint2(lo, hi);
    }
}

// The pair stream of the top level (match_bits.hip: {is-1 dword, is-4 dword} per 32 consecutive bytes of the flat arena).  One thread per
// (phase, position) as in the byte stage; a wave's 64 consecutive positions of a label's plane are 64 consecutive bits of the stream at an
// arbitrary bit offset (planes are not multiples of 32 positions): the ballots are shifted into place and OR-ed into the three dwords
// they touch.  The stream was zeroed by a job of the batch's first launch (fe_job_zero).
static __device__ __forceinline__ void top_bits_body(const int bx, const int by, const LmJob& J, int W, int H, int T, int Wd, int Hd, uint32_t m_wd, uint32_t m_t, uint32_t resp) {
    const int idx = bx * 256 + (int)threadIdx.x;
    const int phase = by, npos = Wd * Hd;
    const bool in = idx < npos;
    uint32_t v = 0;
    if (in) {
        const int ry = (int)fast_div((uint32_t)idx, m_wd, (uint32_t)Wd), rx = idx - ry * Wd;
        const int rs = (int)fast_div((uint32_t)phase, m_t, (uint32_t)T), cs = phase - rs * T;
        v = spread_or(J, rx * T + cs, ry * T + rs, W, H, T);
    }
    uint32_t one;
    resp_planes(v, resp, v, one);                                         // from here on v = "the response is 4", one = "it is the second value"
    const int lane = (int)threadIdx.x & 63;
    const uint32_t idx0 = (uint32_t)(idx - lane);                         // the wave's first position (wave-uniform)
    uint32_t* stream = reinterpret_cast<uint32_t*>(J.lm);                 // pair p: stream[2 p] = is 1, stream[2 p + 1] = is 4
    const uint32_t top_bit0 = (uint32_t)reinterpret_cast<uintptr_t>(J.strips);
    const int plane = lane >= 3, k = lane - 3 * plane;                    // lanes 0..5 carry the three dwords of the two planes
#pragma unroll
    for (int ori = 0; ori < 8; ++ori) {
        const unsigned long long m1 = __ballot(in && ((one >> ori) & 1u)), m4 = __ballot(in && ((v >> ori) & 1u));
        if ((m1 | m4) == 0ull) continue;                                  // wave-uniform
        const uint32_t fo = top_bit0 + (uint32_t)(ori * T * T + phase) * (uint32_t)npos + idx0;   // flat position of the wave's first bit, from the stream's start
        const uint32_t sh = fo & 31u, p0 = fo >> 5;
        const unsigned long long m = plane ? m4 : m1;
        const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
        uint32_t val;
        if (k == 0) val = lo << sh;
        else if (k == 1) val = sh ? (lo >> (32u - sh)) | (hi << sh) : hi;
        else val = sh ? hi >> (32u - sh) : 0u;
        if (lane < 6 && val) atomicOr(stream + 2 * (size_t)(p0 + (uint32_t)k) + (uint32_t)plane, val);
    }
}

// The same when the label planes start on 64-position boundaries of the stream (T * T * positions a multiple of 64: T = 8, or T = 4 with an
// even number of... any grid whose T^2 W_d H_d is): one thread per bit of a label's T * T * positions planes taken as ONE run — phase and
// position follow from the bit index —, a wave = 64 consecutive bits of that run in EVERY label's block, so its ballots are whole dwords:
// lane `label` stores the two pairs {is 1, is 4} x 2 with one 16-byte store.  No atomics, nothing to zero beforehand.
static __device__ __forceinline__ void top_bits_aligned_body(const int bx, const LmJob& J, int W, int H, int T, int Wd, int Hd, uint32_t m_wd, uint32_t m_t, uint32_t m_np, uint32_t resp) {
    const int npos = Wd * Hd, run = T * T * npos;
    const int b = bx * 256 + (int)threadIdx.x;
    const bool in = b < run;
    uint32_t v = 0;
    if (in) {
        const int phase = (int)fast_div((uint32_t)b, m_np, (uint32_t)npos), idx = b - phase * npos;
        const int ry = (int)fast_div((uint32_t)idx, m_wd, (uint32_t)Wd), rx = idx - ry * Wd;
        const int rs = (int)fast_div((uint32_t)phase, m_t, (uint32_t)T), cs = phase - rs * T;
        v = spread_or(J, rx * T + cs, ry * T + rs, W, H, T);
    }
    uint32_t one;
    resp_planes(v, resp, v, one);                                         // v = "the response is 4", one = "it is the second value"
    const int lane = (int)threadIdx.x & 63;
    const uint32_t b0 = (uint32_t)(b - lane);                             // the wave's first bit of the run (a multiple of 64)
    uint4 mine = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int ori = 0; ori < 8; ++ori) {
        const unsigned long long m1 = __ballot(in && ((one >> ori) & 1u)), m4 = __ballot(in && ((v >> ori) & 1u));
        if (lane == ori) mine = make_uint4((uint32_t)m1, (uint32_t)m4, (uint32_t)(m1 >> 32), (uint32_t)(m4 >> 32));
    }
    if (lane < 8 && b0 < (uint32_t)run) {
        const uint32_t pair = ((uint32_t)reinterpret_cast<uintptr_t>(J.strips) + (uint32_t)lane * (uint32_t)run + b0) >> 5;                  // even: the label's block and b0 are multiples of 64 positions
        *reinterpret_cast<uint4*>(J.lm + (size_t)pair * 8) = mine;
    }
}

// The pair stream from pixel TILES (T = 4 or 8, W_d a multiple of 8, the stream's first bit on a byte boundary): a workgroup takes one
// row of cells of one modality.  The 2T - 1 pixel rows its windows touch go to LDS as dwords of four pixels (masked, zero beyond the
// image); the T x T OR of EVERY pixel position of the cell row is separable — along x on the dwords (v_alignbyte), along y on the result —
// so the T x T positions of a cell (= the T x T phases of the linear memory, LL.cpp:1026-1243) share their loads and their ORs instead of
// every (phase, cell) thread loading its own T x T pixels (16 unaligned dword loads for T = 8).  A unit = (phase, 8 neighbouring cells):
// the 8 spread bytes (8 labels x 8 cells) are transposed as an 8 x 8 bit matrix, once for "own bit set" (response 4) and once for
// "only a neighbouring label's" (response 1), which gives for each label the byte of its 8 cells: 16 byte stores, no ballots, no atomics,
// nothing to clear.  (top_bits_aligned_body: 29.5 us per 8-frame batch at VGA — three times the cost per pixel of the level below.)
constexpr int kTileWords = 6144;                 // LDS pool of k_fe_bits (24 KB; 6 workgroups per CU): the staged pixel rows / spread rows / records of the tile writers
static_assert(kTileWords * 2 >= kBitsCells, "the pool holds bits_rows_body's cell words");
static __host__ __device__ inline bool fe_top_tile_fits(int W, int T) { return (T == 4 || T == 8) && (W / T) % 8 == 0 && (3 * T - 1) * (W / 4 + T / 4) <= kTileWords; }
static __host__ __device__ inline int fe_rows_block_rows(int NS, int T);
static __host__ __device__ inline bool fe_rows_tile_fits(int W, int T) { return (T == 4 || T == 5 || T == 8) && W % 16 == 0 && fe_rows_block_rows(((W / T) + 15) / 16, T) > 0; }   // (T = 5: the reference's default step, Detector() = {5, 8})

static __device__ __forceinline__ unsigned long long transpose8x8(unsigned long long x) {      // byte i bit j <-> byte j bit i
    unsigned long long t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull; x = x ^ t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x = x ^ t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x = x ^ t ^ (t << 28);
    return x;
}

// stages of the top level's tile writer: the 2T - 1 pixel rows of cell row ry as dwords (masked, zero beyond the image, RW dwords per row),
// OR-ed along x in place, then along y into s_sp (row rs = the T x T OR of every window that starts in pixel row ry T + rs)
template <int kT>
static __device__ __forceinline__ void tile_spread(const int ry, const LmJob& J, int W, int H, int RW, uint32_t* __restrict__ s_px, uint32_t* __restrict__ s_sp) {
    constexpr int kRows = 2 * kT - 1;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t* q4 = reinterpret_cast<const uint32_t*>(J.quant);
    const uint32_t* m4 = reinterpret_cast<const uint32_t*>(J.mask);
    for (int r = wave; r < kRows; r += 4) {
        const int y = ry * kT + r;
        for (int cw = lane; cw < RW; cw += 64) {
            uint32_t v = 0;
            if (y < H && 4 * cw < W) {
                v = q4[((size_t)y * W >> 2) + cw];
                if (m4) {
                    const uint32_t m = m4[((size_t)y * W >> 2) + cw];
                    const uint32_t nz = ((((m & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | m) & 0x80808080u) >> 7;      // 1 per non-zero mask byte
                    v &= nz * 0xFFu;
                }
            }
            s_px[r * RW + cw] = v;
        }
    }
    __syncthreads();
    // OR of kT consecutive pixels, a wave per row: every lane reads its dwords before any lane of the wave overwrites them
    for (int r = wave; r < kRows; r += 4) {
        for (int c0 = 0; c0 < RW; c0 += 64) {
            const int cw = c0 + lane;
            uint32_t h = 0;
            if (cw < RW) {
                const uint32_t d0 = s_px[r * RW + cw], d1 = cw + 1 < RW ? s_px[r * RW + cw + 1] : 0u;
                h = d0 | __builtin_amdgcn_alignbyte(d1, d0, 1) | __builtin_amdgcn_alignbyte(d1, d0, 2) | __builtin_amdgcn_alignbyte(d1, d0, 3);
                if (kT == 8) {
                    const uint32_t d2 = cw + 2 < RW ? s_px[r * RW + cw + 2] : 0u;
                    h |= d1 | __builtin_amdgcn_alignbyte(d2, d1, 1) | __builtin_amdgcn_alignbyte(d2, d1, 2) | __builtin_amdgcn_alignbyte(d2, d1, 3);
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (cw < RW) s_px[r * RW + cw] = h;
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    for (int i = tid; i < kT * RW; i += 256) {            // ... and of kT consecutive rows
        const int rs = i / RW, cw = i - rs * RW;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < kT; ++k) v |= s_px[(rs + k) * RW + cw];
        s_sp[i] = v;
    }
    __syncthreads();
}

template <int kT>
static __device__ __forceinline__ void top_bits_tile_body(const int ry, const LmJob& J, int W, int H, int Wd, int Hd, uint32_t* __restrict__ s_tile, uint32_t resp) {
    const int RW = W / 4 + kT / 4, tid = (int)threadIdx.x;
    uint32_t* const s_sp = s_tile + (2 * kT - 1) * RW;
    tile_spread<kT>(ry, J, W, H, RW, s_tile, s_sp);
    const int G = Wd >> 3, npos = Wd * Hd, units = kT * kT * G;
    const uint32_t run = (uint32_t)(kT * kT) * (uint32_t)npos, top_bit0 = (uint32_t)reinterpret_cast<uintptr_t>(J.strips);
    const uint8_t* sp = reinterpret_cast<const uint8_t*>(s_sp);
    for (int u = tid; u < units; u += 256) {
        const int phase = u / G, g = u - phase * G;
        const int rs = phase / kT, cs = phase - rs * kT;
        unsigned long long v = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) v |= (unsigned long long)sp[rs * (RW * 4) + (8 * g + j) * kT + cs] << (8 * j);
        uint32_t h0, l0, h1, l1;
        resp_planes((uint32_t)v, resp, h0, l0);
        resp_planes((uint32_t)(v >> 32), resp, h1, l1);
        const unsigned long long t4 = transpose8x8(((unsigned long long)h1 << 32) | h0), t1 = transpose8x8(((unsigned long long)l1 << 32) | l0);
        const uint32_t b = top_bit0 + (uint32_t)phase * (uint32_t)npos + (uint32_t)(ry * Wd + 8 * g);    // bit position (label 0) from the stream's start: a multiple of 8
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const uint32_t bl = b + (uint32_t)l * run;
            uint8_t* o = J.lm + (size_t)(bl >> 5) * 8 + ((bl >> 3) & 3u);
            o[0] = (uint8_t)(t1 >> (8 * l));                   // the pair's "is 1" dword ...
            o[4] = (uint8_t)(t4 >> (8 * l));                   // ... and its "is 4" dword
        }
    }
}

// The strip records of a level below the top from pixel tiles (T = 4, 5 or 8 — 5 is the reference's default step, LL.cpp:1663-1692 —, rows of a multiple of 16 pixels).  A workgroup takes a block of
// R = 16 (or 8) rows of cells of one modality and one pixel-row phase rs; records are [label][phase][strip][row], so R rows of a
// (label, phase, strip) are R x 8 contiguous bytes.
//   A. a wave per row of cells, a lane per four dwords of the row: over the T pixel rows of the windows, the OR of T consecutive pixels starting
//      at each pixel (one 16-byte load + the one or two dwords behind it, masked, zero beyond the image) -> s_sp[row][dword], byte b = the
//      T x T OR of the window at pixel 4 dword + b.  Nothing is staged: every pixel row is read once per phase rs, from L1 / L2.
//   B. per column phase cs: a unit = (16 neighbouring cells, row): per cell the byte "only a neighbouring label's bit" and the byte "own bit" —
//      rows 2c and 2c + 1 of a 32 x 8 bit matrix whose transpose is, per label, exactly the dword {is 1, is 4} x 16 cells of half a record
//      (four 8 x 8 transposes; the interleave is free).  The halves go to LDS as records (half h = low dword of record h, high dword of
//      record h - 1) and leave as 8-byte stores, rows fastest: a wave writes four whole 128-byte lines.
// (bits_rows_body: every (phase, cell) thread loads its own T x T pixels and every record gathers 32 cells with multiplies: 37.7 us per
// 8-frame batch at VGA.  The same tile arithmetic with each unit storing its 16 dwords straight to HBM was as slow: 5.4 M scattered dword stores.)
static __host__ __device__ inline int fe_rows_block_rows(int NS, int T) {       // rows of cells per workgroup: the spread rows + the records of one cs fit the pool
    for (int R = 16; R >= 8; R >>= 1)
        if (R * 4 * T * (NS + 1) + 8 * NS * R * 2 <= kTileWords) return R;
    return 0;
}
template <int kT>
static __device__ __forceinline__ void bits_rows_block_body(const int blk, const int part, const int csn, const LmJob& J, int W, int H, int Wd, int Hd, int NS, uint32_t* __restrict__ s_tile, uint32_t resp) {
    const int rs = part / (kT / csn), cs0 = (part - rs * (kT / csn)) * csn;        // a workgroup takes csn of the kT column phases of its row phase
    const int RW = (NS + 1) * 4 * kT, R = fe_rows_block_rows(NS, kT);       // dwords per spread row: the pixels of 16 NS + 16 cells
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, ry0 = blk * R;
    uint32_t* const s_sp = s_tile;                                         // R x RW
    uint2* const s_rec = reinterpret_cast<uint2*>(s_tile + R * RW);        // [label][strip][row]
    const uint32_t* q4 = reinterpret_cast<const uint32_t*>(J.quant);
    const uint32_t* m4 = reinterpret_cast<const uint32_t*>(J.mask);
    const int W4 = W >> 2;
    auto keep = [](uint32_t m) -> uint32_t { return (((((m & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | m) & 0x80808080u) >> 7) * 0xFFu; };   // 0xFF per non-zero mask byte
    auto px = [&](int y, int cw) -> uint32_t {                             // four pixels of row y, masked; zero beyond the image
        uint32_t v = 0;
        if (cw < W4) {
            v = q4[(size_t)y * W4 + cw];
            if (m4) v &= keep(m4[(size_t)y * W4 + cw]);
        }
        return v;
    };
    for (int rr = wave; rr < R; rr += 4) {
        const int ry = ry0 + rr;
        if (ry >= Hd) break;                                               // (wave-uniform)
        for (int qd = lane; 4 * qd < RW; qd += 64) {
            uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll 4
            for (int k = 0; k < kT; ++k) {
                const int y = ry * kT + rs + k;
                if (y >= H) continue;
                uint32_t d[6] = {0u, 0u, 0u, 0u, 0u, 0u};
                if (4 * qd < W4) {                                         // (rows are multiples of 16 pixels: a quad is inside or outside)
                    const uint4 v = *reinterpret_cast<const uint4*>(q4 + (size_t)y * W4 + 4 * qd);
                    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                    if (m4) {
                        const uint4 m = *reinterpret_cast<const uint4*>(m4 + (size_t)y * W4 + 4 * qd);
                        d[0] &= keep(m.x); d[1] &= keep(m.y); d[2] &= keep(m.z); d[3] &= keep(m.w);
                    }
                }
                d[4] = px(y, 4 * qd + 4);
                if (kT > 5) d[5] = px(y, 4 * qd + 5);
#pragma unroll
                for (int q = 0; q < 4; ++q) {                              // byte b of acc[q]: the OR of the kT pixels from pixel 4 q + b on (kT = 4 .. 8)
                    acc[q] |= d[q] | __builtin_amdgcn_alignbyte(d[q + 1], d[q], 1) | __builtin_amdgcn_alignbyte(d[q + 1], d[q], 2) | __builtin_amdgcn_alignbyte(d[q + 1], d[q], 3);
                    if (kT > 4) acc[q] |= d[q + 1];
                    if (kT > 5) acc[q] |= __builtin_amdgcn_alignbyte(d[q + 2], d[q + 1], 1);
                    if (kT > 6) acc[q] |= __builtin_amdgcn_alignbyte(d[q + 2], d[q + 1], 2);
                    if (kT > 7) acc[q] |= __builtin_amdgcn_alignbyte(d[q + 2], d[q + 1], 3);
                }
            }
            *reinterpret_cast<uint4*>(s_sp + rr * RW + 4 * qd) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
        }
    }
    __syncthreads();
    const uint8_t* sp = reinterpret_cast<const uint8_t*>(s_sp);
    const size_t splane1 = (size_t)NS * Hd * 8;                            // one (label, phase) plane of records
    const int rows = Hd - ry0 < R ? Hd - ry0 : R;
    for (int cs = cs0; cs < cs0 + csn; ++cs) {
        for (int u = tid; u < (NS + 1) * R; u += 256) {
            const int h = u / R, rr = u - h * R;                           // rows fastest
            if (rr >= rows) continue;
            const uint8_t* cell = sp + rr * (RW * 4) + (16 * h) * kT + cs; // the spread byte of cell 16 h + c sits kT bytes further per cell
            unsigned long long t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t v = (uint32_t)cell[(4 * k) * kT] | ((uint32_t)cell[(4 * k + 1) * kT] << 8) | ((uint32_t)cell[(4 * k + 2) * kT] << 16) | ((uint32_t)cell[(4 * k + 3) * kT] << 24);
                uint32_t o;
                resp_planes(v, resp, v, o);                                // v = "is 4", o = "is the second value" (4 1 0 0 0: own bit / only a neighbour's)
                // rows of the bit matrix: o0 v0 o1 v1 | o2 v2 o3 v3
                const uint32_t lo = __builtin_amdgcn_perm(v, o, 0x05010400u), hi = __builtin_amdgcn_perm(v, o, 0x07030602u);
                t[k] = transpose8x8(((unsigned long long)hi << 32) | lo);  // byte l = label l: bits 2c, 2c + 1 of cells 4 k .. 4 k + 3
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {                         // label l: bytes l of t[0..3]
                const uint32_t a0 = (uint32_t)(t[0] >> (32 * half)), a1 = (uint32_t)(t[1] >> (32 * half)), a2 = (uint32_t)(t[2] >> (32 * half)), a3 = (uint32_t)(t[3] >> (32 * half));
                const uint32_t p0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u), p1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
                const uint32_t q0 = __builtin_amdgcn_perm(a3, a2, 0x05010400u), q1 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
                const uint32_t w[4] = {__builtin_amdgcn_perm(q0, p0, 0x05040100u), __builtin_amdgcn_perm(q0, p0, 0x07060302u),
                                       __builtin_amdgcn_perm(q1, p1, 0x05040100u), __builtin_amdgcn_perm(q1, p1, 0x07060302u)};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int l = 4 * half + q;
                    if (h < NS) s_rec[(l * NS + h) * R + rr].x = w[q];
                    if (h > 0) s_rec[(l * NS + h - 1) * R + rr].y = w[q];
                }
            }
        }
        __syncthreads();
        const int phase = rs * kT + cs;
        for (int i = tid; i < 8 * NS * R; i += 256) {
            const int ls = i / R, rr = i - ls * R;                         // ls = label * NS + strip
            if (rr >= rows) continue;
            const int l = ls / NS, st = ls - l * NS;
            *reinterpret_cast<uint2*>(J.lm + ((size_t)l * kT * kT + phase) * splane1 + ((size_t)st * Hd + ry0 + rr) * 8) = s_rec[i];
        }
        __syncthreads();
    }
}

// The bit-plane jobs of a batch (strip records of every level below the top, pair stream of the top level: bits_rows_body, top_bits_body)
// in a launch of their own, the last of the front end: inside k_fe_stage they would cost the colour chain a wave of occupancy (95 VGPRs
// against 79).  Same job table, same persistent walk.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 6)))
k_fe_bits(FeStage st, int total) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[kTileWords];                // one pool for the bodies (a block runs one of them): the cell words of bits_rows_body, the pixel tile of top_bits_tile_body
    for (int blk = (int)blockIdx.x; blk < total; blk += (int)gridDim.x) {
        int j = 0;                                              // (k_fe_stage's decode, restated: fe_device.h says why)
        while (j + 1 < st.njobs && blk >= st.job[j + 1].first) ++j;
        const FeJob& J = st.job[j];
        const int local = blk - J.first;
        const int bz = (int)fast_div((uint32_t)local, J.m_gxgy, (uint32_t)(J.gx * J.gy)), rem = local - bz * J.gx * J.gy;
        const int by = (int)fast_div((uint32_t)rem, J.m_gx, (uint32_t)J.gx), bx = rem - by * J.gx;
        if (J.kind == kFeBitsRows) bits_rows_body(bx, by, J.lm[bz], J.W, J.H, J.a, J.Wd, J.Hd, (J.Wd + 15) >> 4, J.m_wd, J.m_t, reinterpret_cast<uint16_t*>(s_tile), st.resp);
        else if (J.kind == kFeTopBits) top_bits_body(bx, by, J.lm[bz], J.W, J.H, J.a, J.Wd, J.Hd, J.m_wd, J.m_t, st.resp);
        else if (J.kind == kFeTopBitsAligned) top_bits_aligned_body(bx, J.lm[bz], J.W, J.H, J.a, J.Wd, J.Hd, J.m_wd, J.m_t, J.m_np, st.resp);
        else if (J.kind == kFeBitsRowsTile) {
            if (J.a == 8) bits_rows_block_body<8>(bx, by, J.b, J.lm[bz], J.W, J.H, J.Wd, J.Hd, (J.Wd + 15) >> 4, s_tile, st.resp);
            else if (J.a == 5) bits_rows_block_body<5>(bx, by, J.b, J.lm[bz], J.W, J.H, J.Wd, J.Hd, (J.Wd + 15) >> 4, s_tile, st.resp);
            else bits_rows_block_body<4>(bx, by, J.b, J.lm[bz], J.W, J.H, J.Wd, J.Hd, (J.Wd + 15) >> 4, s_tile, st.resp);
        }
        else if (J.kind == kFeTopBitsTile) { if (J.a == 8) top_bits_tile_body<8>(bx, J.lm[bz], J.W, J.H, J.Wd, J.Hd, s_tile, st.resp); else top_bits_tile_body<4>(bx, J.lm[bz], J.W, J.H, J.Wd, J.Hd, s_tile, st.resp); }
        if (blk + (int)gridDim.x < total) __syncthreads();      // the next block of rows reuses the cell words in LDS
    }
}

// strip records of a level below the top, written directly (bits[m]: the level's record block of modality m inside the bit arena)
bool fe_bits_rows_possible(int W, int T) { return fe_bits_rows(W / T) >= 1; }
void fe_job_bits_rows(FeJob& j, const uint8_t* const quant[2], const uint8_t* const mask[2], uint8_t* const bits[2], int W, int H, int T, bool tiles, int m0, int nm) {
    fe_job_lm_grid(j, kFeBitsRows, W, H, T, nm);
    const int R = fe_bits_rows(j.Wd);
    j.gx = (j.Hd + R - 1) / R;
    if (tiles && fe_rows_tile_fits(W, T)) {                // a workgroup per block of rows of cells and pixel-row phase
        const int Rb = fe_rows_block_rows((j.Wd + 15) / 16, T);
        const int k = knobs().fe_rows_cs;
        j.b = k >= 1 && k <= T && T % k == 0 ? k : (T % 2 == 0 ? 2 : 1);   // column phases per workgroup, a divisor of T (LM_FE_ROWS_CS; VGA level 0 at T = 4, per 8-frame batch: all four 23.7 us, two 21.1, one 25.9)
        j.kind = kFeBitsRowsTile; j.gx = (j.Hd + Rb - 1) / Rb; j.gy = T * (T / j.b);
    }
    for (int z = 0; z < nm; ++z) j.lm[z] = LmJob{quant[m0 + z], mask[m0 + z], bits[m0 + z], nullptr};
}
// pair stream of the top level, written directly; bit0[m] = flat arena offset of modality m's block less the stream's first byte
int fe_top_bits_kind(int W, int H, int T, const uint32_t bit0[2], int mode, int m0, int nm) {
    bool bytes = true;                                      // every block written starts on a byte of the stream
    for (int z = 0; z < nm; ++z) bytes = bytes && bit0[m0 + z] % 8 == 0;
    if (mode != 1 && mode != 2 && fe_top_tile_fits(W, T) && bytes) return kFeTopBitsTile;
    if (mode != 1 && ((long)T * T * (W / T) * (H / T)) % 64 == 0) return kFeTopBitsAligned;
    return kFeTopBits;
}
void fe_job_top_bits(FeJob& j, const uint8_t* const quant[2], const uint8_t* const mask[2], uint8_t* stream, const uint32_t bit0[2], int W, int H, int T, int mode, int m0, int nm) {
    fe_job_lm_grid(j, kFeTopBits, W, H, T, nm);
    j.gx = (j.Wd * j.Hd + 255) / 256;
    for (int z = 0; z < nm; ++z) j.lm[z] = LmJob{quant[m0 + z], mask[m0 + z], stream, reinterpret_cast<uint8_t*>((uintptr_t)bit0[m0 + z])};
    const int kind = fe_top_bits_kind(W, H, T, bit0, mode, m0, nm);
    if (kind == kFeTopBitsTile) {                           // a workgroup per row of cells: whole bytes, no atomics, nothing to clear
        j.kind = kFeTopBitsTile; j.gx = j.Hd; j.gy = 1;
    } else if (kind == kFeTopBitsAligned) {                 // whole dwords per wave: no atomics, nothing to clear
        const int npos = j.Wd * j.Hd;
        j.kind = kFeTopBitsAligned; j.gx = (T * T * npos + 255) / 256; j.gy = 1; j.m_np = div_magic((uint32_t)npos);
    }
}
static hipError_t launch_bits_jobs(FeStage& st, hipStream_t s) {
    const int total = fe_prepare(st);
    return total > 0 ? lm_launch(k_fe_bits, dim3(std::min(total, fe_cus() * 8)), dim3(256), 0, s, st, total) : hipSuccess;
}
hipError_t launch_fe_bits(FeStage& st, hipStream_t s) {
    if (!knobs().fe_bits_split) return launch_bits_jobs(st, s);
    for (int kind : {kFeBitsRows, kFeTopBits}) {          // LM_FE_BITS_SPLIT=1 (measurements): the strip-record jobs and the pair-stream jobs as two launches
        FeStage part{};
        part.resp = st.resp;
        for (int i = 0; i < st.njobs; ++i) if ((st.job[i].kind == kFeBitsRows || st.job[i].kind == kFeBitsRowsTile) == (kind == kFeBitsRows)) part.job[part.njobs++] = st.job[i];
        LAUNCH_TRY(launch_bits_jobs(part, s));
    }
    return hipSuccess;
}

}  // namespace lm
