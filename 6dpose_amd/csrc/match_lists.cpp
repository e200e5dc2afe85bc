// Result lists on the host: the canonical merge, the reference's own output order, and the drivers' NMS routines.  Pure CPU code.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "detector_internal.h"

// ---- canonical merge (LL.cpp:1771-1776 with the total order of SURVEY A12) ---------------------------
static bool match_less(const lm_match& a, const lm_match& b) {
    if (a.similarity != b.similarity) return a.similarity > b.similarity;
    if (a.template_id != b.template_id) return a.template_id < b.template_id;
    if (a.class_index != b.class_index) return a.class_index < b.class_index;
    if (a.y != b.y) return a.y < b.y;
    return a.x < b.x;
}
static bool match_eq(const lm_match& a, const lm_match& b) {   // Match::operator== (LL.h:243-246)
    return a.x == b.x && a.y == b.y && a.similarity == b.similarity && a.class_index == b.class_index;
}
// LSD radix sort on the 112-bit key (~similarity bits, template_id | class, y, x), 11-bit digits,
// digits that are constant over the input are skipped.  Equivalent to std::sort(match_less).
// distinct_input: the records hold no exact duplicates (k_dedupe removed them on the device): the hash pass is skipped.
// Scratch buffers are per thread and reused (a frame's list is merged in ~20 us; six allocations were a third of it).
size_t merge_matches_impl(lm_match* m, size_t n, bool distinct_input) {
    if (!m || n == 0) return 0;
    if (n < 64) {
        std::sort(m, m + n, match_less);
        return (size_t)(std::unique(m, m + n, match_eq) - m);
    }
    struct Key { uint64_t hi, lo; };
    static thread_local std::vector<Key> keys;
    static thread_local std::vector<uint32_t> idx, tmp, table;
    static thread_local std::vector<lm_match> out;
    keys.resize(n);
    bool radix_ok = true;
    for (size_t i = 0; i < n; ++i) {
        uint32_t sb;
        memcpy(&sb, &m[i].similarity, 4);
        if ((sb >> 31) || m[i].similarity != m[i].similarity || m[i].template_id < 0 || m[i].class_index < 0 || m[i].class_index > 0xFFFF ||
            m[i].x < -32768 || m[i].x > 32767 || m[i].y < -32768 || m[i].y > 32767) { radix_ok = false; break; }
        if (sb == 0x80000000u) sb = 0;
        keys[i].hi = ((uint64_t)(~sb) << 32) | (uint32_t)m[i].template_id;
        keys[i].lo = ((uint64_t)m[i].class_index << 32) | ((uint64_t)(uint16_t)(m[i].y + 32768) << 16) | (uint16_t)(m[i].x + 32768);
    }
    if (!radix_ok) {   // negative / NaN similarities or out-of-range fields: comparison sort
        std::sort(m, m + n, match_less);
        return (size_t)(std::unique(m, m + n, match_eq) - m);
    }
    idx.clear();
    idx.reserve(n);
    if (distinct_input) {
        for (size_t i = 0; i < n; ++i) idx.push_back((uint32_t)i);
    } else {
        // Exact duplicates (same x, y, similarity, class AND template: several coarse candidates of one
        // template refined to the same position) are adjacent in the canonical order and removed by the
        // unique step anyway: drop them first with an open-addressing hash so that the sort sees ~n/5.
        size_t cap = 64;
        while (cap < 2 * n) cap <<= 1;
        table.assign(cap, 0xFFFFFFFFu);
        for (size_t i = 0; i < n; ++i) {
            uint64_t h = (keys[i].hi * 0x9E3779B97F4A7C15ull) ^ (keys[i].lo * 0xC2B2AE3D27D4EB4Full);
            size_t slot = (size_t)(h ^ (h >> 29)) & (cap - 1);
            for (;;) {
                uint32_t j = table[slot];
                if (j == 0xFFFFFFFFu) { table[slot] = (uint32_t)i; idx.push_back((uint32_t)i); break; }
                if (keys[j].hi == keys[i].hi && keys[j].lo == keys[i].lo) break;
                slot = (slot + 1) & (cap - 1);
            }
        }
    }
    const size_t nu = idx.size();
    tmp.resize(nu);
    constexpr int BITS = 11, NB = 1 << BITS;
    uint32_t hist[NB];
    // which bits vary at all: digits whose bits are constant over the input need no pass (and no histogram)
    uint64_t or_lo = 0, and_lo = ~0ull, or_hi = 0, and_hi = ~0ull;
    for (size_t i = 0; i < nu; ++i) { const Key& k = keys[idx[i]]; or_lo |= k.lo; and_lo &= k.lo; or_hi |= k.hi; and_hi &= k.hi; }
    const uint64_t var_lo = or_lo ^ and_lo, var_hi = or_hi ^ and_hi;
    for (int word = 0; word < 2; ++word)          // lo word first (least significant)
        for (int shift = 0; shift < (word == 0 ? 48 : 64); shift += BITS) {
            if ((((word == 0 ? var_lo : var_hi) >> shift) & (NB - 1)) == 0) continue;   // constant digit
            memset(hist, 0, sizeof(hist));
            for (size_t i = 0; i < nu; ++i) {
                uint64_t k = word == 0 ? keys[idx[i]].lo : keys[idx[i]].hi;
                ++hist[(k >> shift) & (NB - 1)];
            }
            uint32_t sum = 0;
            for (int b = 0; b < NB; ++b) { uint32_t c = hist[b]; hist[b] = sum; sum += c; }
            for (size_t i = 0; i < nu; ++i) {
                uint32_t id = idx[i];
                uint64_t k = word == 0 ? keys[id].lo : keys[id].hi;
                tmp[hist[(k >> shift) & (NB - 1)]++] = id;
            }
            idx.swap(tmp);
        }
    out.clear();
    out.reserve(nu);
    for (size_t i = 0; i < nu; ++i) {
        const lm_match& c = m[idx[i]];
        if (out.empty() || !match_eq(out.back(), c)) out.push_back(c);
    }
    memcpy(m, out.data(), out.size() * sizeof(lm_match));
    return out.size();
}
extern "C" size_t lm_merge_matches(lm_match* m, size_t n) { return merge_matches_impl(m, n, false); }

// The reference's own output, permutation and surviving duplicates included (sort_unique 3 / lm_detector_set_reference_order).
// Detector::match ends with std::sort under an order that ignores x, y and std::unique under an equality that ignores
// template_id (LL.cpp:1771-1776, LL.h:234-246): what comes out depends on the order the records went in and on
// libstdc++'s introsort.  Both are reproducible: the reference appends class by class (caller's order), template by
// template, candidates in raster order of the coarse grid (LL.cpp:1753-1769, 1835-1852; remove_if keeps the order) — the
// coarse position of every slot is in the candidate buffer — and std::sort is the same template of the same libstdc++
// this library is built with, so the same comparisons on the same sequence give the same permutation.
// recs / coarse: the ncand raw records of a frame and their coarse candidates; alive: how many records survive (a hint for the
// allocation); wcls / wtid: class position and template id per work item.  Returns the malloc'ed list (null: out of memory).
lm_match* reference_order_list(const Candidate* recs_in, const Candidate* coarse, uint64_t ncand, size_t alive, const std::vector<int32_t>& wcls,
                               const std::vector<int32_t>& wtid, size_t* n_out, ListClock* clock) {
    struct Rec { int32_t cls, tid, cy, cx; lm_match m; };
    std::vector<Rec> recs;
    recs.reserve(alive);
    for (uint64_t i = 0; i < ncand; ++i) {
        const Candidate& c = recs_in[i];
        if (c.work < 0) continue;
        Rec r;
        r.cls = wcls[c.work]; r.tid = wtid[c.work]; r.cy = coarse[i].y; r.cx = coarse[i].x;
        r.m.x = c.x; r.m.y = c.y; r.m.similarity = c.score; r.m.class_index = r.cls; r.m.template_id = r.tid;
        recs.push_back(r);
    }
    std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) {      // a total order: emission order of the reference
        if (a.cls != b.cls) return a.cls < b.cls;
        if (a.tid != b.tid) return a.tid < b.tid;
        if (a.cy != b.cy) return a.cy < b.cy;
        return a.cx < b.cx;
    });
    clock->converted = std::chrono::steady_clock::now();
    std::vector<lm_match> v(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) v[i] = recs[i].m;
    std::sort(v.begin(), v.end(), [](const lm_match& a, const lm_match& b) {  // Match::operator< (LL.h:234-241)
        if (a.similarity != b.similarity) return a.similarity > b.similarity;
        return a.template_id < b.template_id;
    });
    v.erase(std::unique(v.begin(), v.end(), match_eq), v.end());               // Match::operator== (LL.h:243-246)
    clock->merged = std::chrono::steady_clock::now();
    lm_match* res = (lm_match*)malloc(std::max<size_t>(1, v.size()) * sizeof(lm_match));
    if (!res) return nullptr;
    if (!v.empty()) memcpy(res, v.data(), v.size() * sizeof(lm_match));
    *n_out = v.size();
    return res;
}

// numpy nms of the driver (linemod_and_levelup_test.py:34-61)
extern "C" int lm_nms_boxes(const double* boxes, const double* scores, int n, double thresh, int32_t* keep) {
    if (n <= 0 || !boxes || !scores || !keep) return 0;
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[i] = i;
    // scores.argsort()[::-1]: ascending stable-ish sort reversed -> among equal scores higher index first
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return scores[a] < scores[b]; });
    std::reverse(order.begin(), order.end());
    std::vector<char> dead((size_t)n, 0);
    int kept = 0;
    for (int oi = 0; oi < n; ++oi) {
        int i = order[oi];
        if (dead[i]) continue;
        keep[kept++] = i;
        double ai = (boxes[4 * i + 2] - boxes[4 * i] + 1) * (boxes[4 * i + 3] - boxes[4 * i + 1] + 1);
        for (int oj = oi + 1; oj < n; ++oj) {
            int j = order[oj];
            if (dead[j]) continue;
            double xx1 = std::max(boxes[4 * i], boxes[4 * j]), yy1 = std::max(boxes[4 * i + 1], boxes[4 * j + 1]);
            double xx2 = std::min(boxes[4 * i + 2], boxes[4 * j + 2]), yy2 = std::min(boxes[4 * i + 3], boxes[4 * j + 3]);
            double w = std::max(0.0, xx2 - xx1 + 1), h = std::max(0.0, yy2 - yy1 + 1);
            double inter = w * h;
            double aj = (boxes[4 * j + 2] - boxes[4 * j] + 1) * (boxes[4 * j + 3] - boxes[4 * j + 1] + 1);
            double ovr = inter / (ai + aj - inter);
            if (!(ovr <= thresh)) dead[j] = 1;
        }
    }
    return kept;
}

// Translation NMS over refined poses (linemod_ros/detect.py:41-51, `nms_norms(ts, ts_scores, 40.0)` at :128): visit by
// score descending, keep, drop every later pose whose translation is within `thresh` of it (kept iff ||t_i - t_j|| > thresh,
// double precision, numpy's sqrt(dx*dx + dy*dy + dz*dz)).  Visiting order among EQUAL scores: the higher index first — what
// `scores.argsort()[::-1]` gives for n <= 16 (numpy's default argsort is an introsort: insertion sort, hence stable, up to 16
// elements; beyond that numpy's tie order is an implementation detail and this function's rule is this library's definition, not a
// reference-exact one).
extern "C" int lm_nms_norms(const double* ts, const double* scores, int n, double thresh, int32_t* keep) {
    if (n <= 0 || !ts || !scores || !keep) return 0;
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return scores[a] < scores[b]; });
    std::reverse(order.begin(), order.end());
    std::vector<char> dead((size_t)n, 0);
    int kept = 0;
    for (int oi = 0; oi < n; ++oi) {
        const int i = order[oi];
        if (dead[i]) continue;
        keep[kept++] = i;
        for (int oj = oi + 1; oj < n; ++oj) {
            const int j = order[oj];
            if (dead[j]) continue;
            const double dx = ts[3 * i] - ts[3 * j], dy = ts[3 * i + 1] - ts[3 * j + 1], dz = ts[3 * i + 2] - ts[3 * j + 2];
            const double norm = sqrt(dx * dx + dy * dy + dz * dz);
            if (!(norm > thresh)) dead[j] = 1;
        }
    }
    return kept;
}

// cv::dnn::NMSBoxes(std::vector<Rect>, scores, score_threshold, nms_threshold, indices, eta, top_k) as linemodLevelup/test.cpp:
// 132-144 uses it (40x40 boxes at the match positions, score_threshold 0, nms_threshold 0.4).  OpenCV is un-vendored and its
// version unpinned; this follows the published algorithm of OpenCV 3.4's dnn/src/nms.inl.hpp (NMSFast_): candidates with
// score > score_threshold, std::stable_sort by score descending (ties keep input order), optional top_k cut, then greedily keep
// a box iff its overlap with every box kept so far is <= the adaptive threshold (which shrinks by eta after each keep while
// > 0.5 and eta < 1).  overlap = 1.f - float(jaccardDistance(a, b)), jaccardDistance in double on integer rectangle areas,
// 0 when both are empty.  rects: [n][4] int32 x, y, width, height.
extern "C" int lm_nms_boxes_cv(const int32_t* rects, const float* scores, int n, float score_threshold, float nms_threshold, float eta,
                               int top_k, int32_t* keep) {
    if (n <= 0 || !rects || !scores || !keep) return 0;
    std::vector<int> order;
    for (int i = 0; i < n; ++i) if (scores[i] > score_threshold) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return scores[a] > scores[b]; });
    if (top_k > 0 && (size_t)top_k < order.size()) order.resize((size_t)top_k);
    auto overlap = [&](int a, int b) -> float {
        const int32_t* A = rects + 4 * a; const int32_t* B = rects + 4 * b;
        const double Aa = (double)A[2] * A[3], Ab = (double)B[2] * B[3];
        if ((Aa + Ab) <= 2.220446049250313e-16) return 1.f - 0.f;                       // jaccardDistance: "identical": distance 0
        const int x1 = std::max(A[0], B[0]), y1 = std::max(A[1], B[1]);
        const int x2 = std::min(A[0] + A[2], B[0] + B[2]), y2 = std::min(A[1] + A[3], B[1] + B[3]);
        const double Aab = (x2 > x1 && y2 > y1) ? (double)(x2 - x1) * (y2 - y1) : 0.0;     // (a & b).area(): empty unless both extents positive
        return 1.f - (float)(1.0 - Aab / (Aa + Ab - Aab));
    };
    float adaptive = nms_threshold;
    int kept = 0;
    for (int idx : order) {
        bool ok = true;
        for (int k = 0; k < kept && ok; ++k) ok = overlap(idx, keep[k]) <= adaptive;
        if (ok) keep[kept++] = idx;
        if (ok && eta < 1.f && adaptive > 0.5f) adaptive *= eta;
    }
    return kept;
}
