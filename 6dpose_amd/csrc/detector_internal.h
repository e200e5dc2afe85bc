// Private view of the detector shared by the detector's translation units (detector.cpp, detector_frame.cpp, detector_bank.cpp,
// detector_frontend.cpp, detector_launch.cpp, detector_collect.cpp, detector_ingest.cpp, detector_slabs.cpp, detector_scaled.cpp, host_pool.cpp,
// match_lists.cpp), bank_file.cpp, comm.cpp, exchange.cpp and pipeline.cpp (not part of the C ABI).
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/amd_linemod.h"
#include "depth_modes.h"
#include "dev_buf.h"
#include "frame_border.h"
#include "host_templates.h"
#include "knobs.h"
#include "launch_model.h"
#include "lm_kernels.h"
#include "scaled_kernels.h"

namespace lm {}
using namespace lm;

struct LevelBufs {
    int W = 0, H = 0;
    DevBuf<uint8_t> rgb;      // level>0 only (level 0 aliases the frame)
    DevBuf<float> mag;
    DevBuf<uint8_t> ang;      // one-hot quantised orientation (unmasked)
    DevBuf<uint8_t> nrm;      // one-hot quantised normal (unmasked)
    DevBuf<uint8_t> mask[2];  // per modality, optional
};

// What the linear-memory and bit-plane jobs of the front end take for one level of one frame (lm_detector::level_ptrs)
struct LevelPtrs {
    const uint8_t* quant[2];  // quantised maps: [0] colour, [1] normals
    const uint8_t* mask[2];   // null where the slot's frame came without that mask
    uint8_t* lm[2];           // flat linear memories
    uint8_t* strips[2];       // their strip-major copy (null at the top level)
    uint8_t* bits[2];         // strip records (null at the top level)
    uint8_t* top_stream;      // pair stream of the slot; bit0[m] = modality m's block in it (meaningful at the top level)
    uint32_t bit0[2];
};

struct lm_detector {
    // device.  The four streams come first, before every event and every DevBuf / PinBuf of the detector (dev_buf.h: members die in
    // reverse order, so the buffers are freed and the events destroyed while all four streams still exist), and in the order in which
    // lm_detector_create creates them.
    int device = 0;
    DevStream stream;                   // frame upload / select + front end (and addTemplate)
    DevStream mstream;                  // refinement (a lone frame: all three matching kernels; + the pipeline's NMS / ICP): frame k, while `stream` prepares frame k+1
    DevStream xchg_stream;              // multi-GPU exchange (exchange.cpp); also runs the duplicate removal of pipelined frames
    DevStream ingest_stream;            // copy stream of the live-stream ingest; created with the detector, or by the first streamed frame if that failed
    DevEvent ev[8];
    int shard_rank = 0, shard_world = 1;

    // parameters (LL.cpp:1663-1692 + modality defaults :645-650, :968-974)
    int num_features = 63;
    std::vector<int> T_at_level{5, 8};
    int pyramid_levels = 2;
    float weak_threshold = 10.0f, strong_threshold = 55.0f;
    int distance_threshold = 2000, difference_threshold = 50, extract_threshold = 2;
    TemplatesMap class_templates;
    // The modality set, fixed at creation (lm_detector_create_modalities): kind 0 = ColorGradient, 1 = DepthNormal.  mod_kind[i] is the kind of the
    // set's i-th modality (the order of sources, masks and of the templates of a pyramid level); use[k] says whether kind k is in the set.  Device
    // buffers, arena blocks and LevelPtrs stay indexed by KIND: a set of one leaves the other kind's blocks allocated, zero and never written.
    int nmod = 2;
    int mod_kind[2] = {0, 1};
    bool use[2] = {true, true};
    // Channels of the colour image (lm_detector_set_colour_channels): 3, or 1 for a grey camera.  Sizes every colour buffer, staging slice and upload,
    // and selects the front end's grey job kinds; nothing downstream of the quantised maps sees it.
    int cch = 3;

    // Frames of any size (lm_detector_set_border): kBorderStrict refuses a source size that is not aligned (the reference's
    // asserts), kBorderPad / kBorderCrop extend or cut it at the right and bottom to the aligned size of border_aligned_size.  Two geometries
    // from there on: the SOURCE size is what the caller hands over, what the pinned staging and the ingest ring's host entries hold and what
    // crosses PCIe; the ALIGNED size (fW x fH, geom) is that of the frame buffers, the arenas, the parked frames and lm_detector_read_stage.
    int border = kBorderStrict;
    DevBuf<uint8_t> border_src;         // the uploaded sources (and masks) of a blocking upload whose size is not aligned: k_frame_border reads them

    // frame
    int fW = 0, fH = 0;
    bool frame_valid = false, have_mask[2] = {false, false};
    DevBuf<uint8_t> frame_rgb;
    DevBuf<uint16_t> frame_depth;
    const uint8_t* cur_rgb = nullptr;           // what the front end reads: frame_rgb / frame_depth, or — for a frame that came in through
    const uint16_t* cur_depth = nullptr;        // lm_detector_submit_frame — the ingest ring's device buffers (no device-to-device copy)
    DevBuf<uint8_t> nrm_raw;                    // normals before the median (level 0)
    static constexpr int kSlots = 16;           // frames in flight (lm_detector_submit / collect; lm_detector_max_in_flight): every one owns
                                                // its arenas, candidate / record buffers and pinned result memory (~35 MB at VGA)
    DevBuf<uint8_t> lm_arena[kSlots], sm_arena[kSlots];   // linear memories per result slot: the front end of frame k+1 writes one set
                                                // while the matching kernels of frame k read the other
    int last_arena = 0;                         // set written by the most recent front end (lm_detector_read_stage)
    bool quantised = false;                     // a front end has written lvl[]'s quantised maps at the current frame size (lm_pso_set_scene_from_detector)

    LevelBufs lvl[kMaxLevels];                  // front-end intermediates of frame 0 of a batch (and of addTemplate, read_stage)
    LevelBufs lvl_x[kMaxBatch - 1][kMaxLevels]; // ... of frames 1.. of a batch (allocated on first use)
    DevBuf<uint8_t> nrm_raw_x[kMaxBatch - 1];
    LevelBufs& level_bufs(int b, int l) { return b == 0 ? lvl[l] : lvl_x[b - 1][l]; }
    FrameGeom geom{};
    size_t lm_block_bytes[kMaxLevels] = {};
    std::vector<DevBuf<uint8_t>> slot_rgb;      // frames parked in HBM (lm_detector_store_frame)
    std::vector<DevBuf<uint16_t>> slot_depth;
    std::vector<int> slot_w, slot_h;
    PinBuf<uint8_t> pinned;          // staging for H2D frame and D2H results
    float last_h2d_ms = 0.f;

    // bank on device
    bool bank_dirty = true;
    int bank_geom_W = -1, bank_geom_H = -1;
    std::vector<std::string> bank_classes;          // sorted
    std::vector<int> bank_class_base;               // first flat pyramid index per class
    std::vector<int> bank_class_count;
    std::vector<TemplEntry> h_entries;
    DevBuf<TemplEntry> d_entries;
    DevBuf<int32_t> d_feat_off;
    DevBuf<uint32_t> d_feat_xy;
    DevBuf<uint32_t> d_feat_word, d_run_mask;       // refinement levels: feature words + class-run masks (lm_kernels.h)
    // Part-based matching (lm_detector_set_part_matching; match_parts.hip): off while part_min_parts == 0.  Switched on, upload_bank
    // also builds the part table of every entry and the part-ordered copies of feat_off / feat_word (one index space, like the holistic arrays).
    int part_min_parts = 0, part_min_features = 8;
    DevBuf<PartEntry> d_parts;
    DevBuf<int32_t> d_part_off;
    DevBuf<uint32_t> d_part_word;
    // work list
    std::vector<int32_t> work_pyr;
    std::shared_ptr<std::vector<int32_t>> work_cls, work_tid;   // shared with in-flight result slots
    DevBuf<int32_t> d_work;
    std::vector<std::string> work_key;              // class_ids the cached work list was built for
    int work_key_rank = -1, work_key_world = -1;
    bool work_valid = false;
    int64_t work_coarse_bytes = 0;
    DevBuf<Candidate> d_cands;
    DevBuf<Candidate> d_matches_dev;                // HBM copy of the refined records (on-device NMS / top-K, duplicate removal)
    DevBuf<unsigned long long> d_hash;              // open-addressing table of k_dedupe
    DevBuf<TileRec> d_tiles;                        // per result slot: the tiles k_coarse planned (cand_cap / 2 records each)
    DevBuf<uint8_t> d_todo;                         // per result slot: 1 = candidate that no tile serves (refined on its own)
    bool use_tiles = true;                          // LM_TILES=0: every candidate on its own (the round-1 refinement)
    bool reference_order = false;                   // lm_detector_set_reference_order / LM_REFERENCE_ORDER=1: match() returns the reference's own permutation (sort_unique 3)
    DevBuf<ulonglong2> d_distinct_keys;             // the distinct records as 128-bit sort keys, per result slot (multi-GPU exchange)
    DevBuf<int32_t> d_work_cls, d_work_tid;         // class position / template id per work item
    DevBuf<unsigned long long> d_counters;          // kCounterWords working counters per result slot: zero between frames (k_dedupe's last block resets them)
    DevBuf<unsigned long long> d_final;             // per result slot: [0] candidates, [1] distinct, [2] alive, [3] key overflow of the finished frame
    uint32_t cand_cap = 1u << 18;                   // candidate capacity wanted (raised when a frame overflowed)
    uint32_t buf_cand_cap = 0;                      // ... the per-slot device buffers are laid out for (frames in flight use this one)
    // Result slots: the refinement kernel of a later frame writes into one pinned buffer while the host
    // collects an earlier frame from another (lm_detector_submit / lm_detector_collect).
    struct Slot {
        PinBuf<Candidate> h_matches;                // the raw records, copied from matches_dev when a collect asks for them
        PinBuf<Candidate> h_distinct;               // the same without exact duplicates (k_dedupe), unordered; as many as h_matches
        PinBuf<unsigned long long> h_counters;      // [0] candidate count, [1] distinct records, [2] records alive, [8..] 2 words of statistics per refinement block
        // A BATCH of consecutive slots is launched together (one front end / coarse / refinement / duplicate-removal launch for all
        // its frames); the events below are those of the batch's first slot (`leader`).
        int leader = -1, batch_n = 1;               // first slot of the batch this frame was launched with, frames in that batch
        bool launched = false;                      // false: submitted but still waiting for its batch to fill (lm_detector_flush / collect launch it)
        const uint8_t* in_rgb = nullptr;            // the frame the front end reads: the detector's resident frame or the slot's ingest ring entry
        const uint16_t* in_depth = nullptr;
        bool have_mask[2] = {false, false};         // lone frames only (Detector.match with masks)
        int ring = -1;                              // ingest ring entry holding the frame (-1: resident frame)
        int src_w = 0, src_h = 0;                   // != 0: the ring entry holds the frame at this source size; the batch's k_frame_border writes the aligned frame the front end reads
        bool src_in_place = false;                  // ... its rows are in the aligned buffers already (2-D copies), only the margins are missing
        // prepared by the collector thread (streamed frames): the frame's Detector::match list, ready when `ready` != 0
        bool prep_queued = false;                   // a collector job covers this frame
        std::atomic<int> ready{0};                  // 0 not yet, 1 list prepared, 2 nothing prepared (overflow: the caller's path decides)
        lm_match* prep = nullptr;
        size_t prep_n = 0;
        float prep_collect_ms = 0.f, prep_merge_ms = 0.f;
        DevEvent ev[6];                             // stage timing: front end 0 -> 1, coarse 1 -> 3, refinement 3 -> 4 (2 and 5: not recorded since round 5)
        DevEvent done;                              // recorded after the batch's last kernel: the only event the host waits on
        DevEvent fe_done;                           // front end of this slot finished (eager, on `stream`): `mstream` waits for it
        bool pending = false;
        float threshold = 0.f, h2d_ms = 0.f;
        int num_work = 0;
        uint32_t cand_cap = 0;                      // the candidate capacity / buffer this frame was submitted with (d->cand_cap may grow before it is collected)
        const Candidate* cands = nullptr;
        const Candidate* matches_dev = nullptr;     // the frame's refined records in HBM (one per candidate, work = -1: dropped)
        int64_t coarse_bytes = 0;
        std::shared_ptr<std::vector<int32_t>> work_cls, work_tid;
        std::chrono::steady_clock::time_point t0, t1;
    } slot[kSlots];
    // Bit planes (match_bits.hip): both matching kernels read 1-bit response planes by default.
    DevBuf<uint8_t> cbits_arena[kSlots];            // pair stream of the top level's flat memories (k_coarse_bits)
    uint32_t cbits_byte0 = 0, cbits_npairs = 0;     // ... = arena bytes [byte0, byte0 + 32 npairs): the top level's two blocks with their zero tails
    DevBuf<uint8_t> bits_arena[kSlots];             // strip records of the levels below the top (the strip arena's layout at half the offsets; k_local_bits)
    int bits_max_nf = 0, cbits_max_nf = 0;          // largest feature count of a template entry below the top level / at the top level (which counter width the kernels need)
    bool bits_all_in = false;                       // every candidate's windows lie inside their planes at every level: k_local_bits leaves nothing to k_local
    // Which kernels match() uses (lm_detector_set_paths; tests and measurements of the byte paths).  refine: 0 = bit planes when the pyramid has a
    // level below the top (default), 1 = byte strip planes with tiles (round 2-3's k_local), 2 = byte planes, every candidate on its own
    // (round 1).  coarse: 0 = pair stream when the refinement runs on bit planes (default), 1 = byte linear memories (k_coarse).
    // refine 3 / coarse 2 = "wide": what 0 is for a table of two planes, and two sets of bit planes (match_wide.hip) for the tables that need them.
    int refine_mode = 0, coarse_mode = 0;
    int coarse_batch = knobs().coarse_batch;        // lm_detector_set_coarse_batch: k_coarse_bits (0), k_coarse_bits_batch (1) or the launcher's rule (-1) for the coarse pass on the pair stream
    bool coarse_batched = false;                    // the last such coarse pass ran k_coarse_bits_batch (lm_detector_get_coarse_batch)
    // Second set of bit planes of the wide paths, per result slot: allocated (and zeroed) when a batch first runs a wide table on a wide path,
    // at the sizes of bits_arena / cbits_arena; a geometry change resizes and clears the ones that exist (setup_geometry).
    DevBuf<uint8_t> wbits_arena[kSlots], wcbits_arena[kSlots];
    // The response table r[d], d = cyclic distance 0..4 (lm_detector_set_response_table; LL.cpp:1112-1124).  Per detector and per process: no file
    // format carries it, training does not read it.  Every front end launch takes it along (FeStage::resp), so the next match of the resident frame
    // rebuilds the response memories under the new table.  Tables with more than two distinct non-zero values run on the byte kernels.
    uint8_t resp_table[5] = {4, 1, 0, 0, 0};
    uint32_t resp = kRespDefault;                   // resp_pack(resp_table)
    int resp_low_weight = 1;                        // the weight a of the bit-plane kernels' low plane
    bool resp_two_planes = true;                    // at most two distinct non-zero values: the bit-plane kernels serve the table
    bool fe_direct = true;                          // lm_detector_set_direct_bits: the front end writes bit planes directly where nothing reads the bytes (0: bytes + k_pack_bits / k_pack_top)
    bool fe_keep_top = false;                       // lm_detector_set_direct_bits(d, 2)
    int fe_top_mode = 0;                            // lm_detector_set_direct_bits(d, 4 / 8): which writer of the pair stream (fe_job_top_bits)
    bool fe_bytes_low = true, fe_bytes_top = true;  // did the last front end write the byte planes of the levels below the top / of the top level (read_stage builds them on demand otherwise)
    hipEvent_t resident_reader = nullptr;           // front end (event of its batch) that reads the resident frame buffers: lm_detector_select_frame's copy waits for it (not owned: a slot's fe_done)
    // frame b of a batch (its intermediates: level_bufs), level l, result slot `arena` (whose frame decides the masks)
    LevelPtrs level_ptrs(int b, int l, int arena) {
        const LevelBufs& q = level_bufs(b, l);
        const LevelGeom& lv = geom.lv[l];
        const bool low = l < pyramid_levels - 1;
        LevelPtrs P{};
        P.quant[0] = q.ang.p; P.quant[1] = q.nrm.p;
        for (int m = 0; m < 2; ++m) {
            P.mask[m] = slabs.mask_on ? slabs.mask_of[l][m] : (slot[arena].have_mask[m] ? lvl[l].mask[m].p : nullptr);
            P.lm[m] = lm_arena[arena].p + lv.lm_off[m];
            P.strips[m] = low ? sm_arena[arena].p + lv.sm_off[m] : nullptr;
            P.bits[m] = low ? bits_arena[arena].p + (lv.sm_off[m] >> 1) : nullptr;
            P.bit0[m] = lv.lm_off[m] - cbits_byte0;
        }
        P.top_stream = cbits_arena[arena].p;
        return P;
    }
    // Depth slabs (detector_slabs.cpp).  The histogram, the mode records and the slab masks live on the device; a pass of
    // lm_detector_match_slabs under a slab sets mask_on, and the front end's writers then take mask_of[level][kind] — the slab ANDed with the
    // user's mask of that modality, or the slab alone — instead of the resident frame's own masks, which are never written.  quantised: the
    // quantised maps of lvl[] are those of the resident frame already, so the front end of a lone frame only builds its response memories.
    struct Slabs {
        DevBuf<uint32_t> hist, modes;               // kDepthMaxBins counts; kDepthModeWords words of mode records
        PinBuf<uint32_t> h_modes;                   // copy of the mode records
        DevEvent modes_ready;                       // created by the first pass (enqueue_modes)
        DevBuf<uint8_t> mask[kMaxLevels][3];        // [level][0 / 1: slab & user mask of that kind, 2: the slab alone]
        const uint8_t* mask_of[kMaxLevels][2] = {};
        bool mask_on = false, quantised = false;
    } slabs;
    std::map<std::string, std::pair<int, int>> class_depth_range;   // lm_detector_set_class_depth_range: host state, stored in no file
    // Depth-scaled matching (detector_scaled.cpp; match_scaled.hip): the training depth of a class (host state, stored in no
    // file, like the depth ranges), and what a call keeps between calls: the probe map, the K-row tables of the selected classes — cached per
    // (bank generation, ladder, selection) — and candidate buffers of its own (`cap` starts at cand_cap and grows when a call overflows it).
    std::map<std::string, int> class_train_depth;
    uint64_t bank_generation = 0;                   // counts upload_bank: a bank or geometry change
    int pipelines = 0;                              // lm_pipeline objects created on this detector and not destroyed
    struct Scaled {
        DevBuf<uint16_t> probe;
        DevBuf<ScaledFeat> table;
        DevBuf<ScaledEntry> entries;
        DevBuf<int32_t> train;
        DevBuf<ScaledCand> cands;
        DevBuf<unsigned int> counter;
        uint32_t cap = 0;
        bool table_valid = false;
        uint64_t key_generation = 0;
        std::vector<int32_t> key_ladder;
        std::vector<std::string> key_classes;
        int max_nf_top = 0;
    } scaled;
    bool cbits_clean[kSlots] = {};                  // the slot's pair stream is all zero (what the front end's OR-ing writer needs)
    uint64_t n_submitted = 0, n_collected = 0, n_launched = 0;
    // frames submitted but not launched yet: slots pend_first .. pend_first + pend_n - 1 (modulo kSlots), same threshold and work list
    int pend_first = 0, pend_n = 0;
    float pend_threshold = 0.f;
    // When a streamed frame that does not fill its batch goes out (launch_model.h): the queue of launched batches, the clocks and moving
    // averages, and the knobs batch_max (lm_detector_set_batch), keep_queued (lm_detector_set_batch_queue), first_batch and launch_slack_ms.
    LaunchModel launch;
    // Helper threads of the streamed path (one pool per detector, started with the first job; LM_HOST_THREADS, default 3, 0 = none).  They
    // never call into the HIP runtime — a second thread inside the runtime made every HIP call of the calling thread take ~0.1 ms (round 3:
    // the collector thread that waited on events) — and do two things:
    //   * the staging copy of a streamed frame (1.5 MB at VGA: 40 us on one core) in slices, beside the caller's own slice;
    //   * the canonical result lists: frames are launched in batches, so when the collect of a batch's first frame has seen the batch's
    //     event, the records of ALL its frames are in pinned memory — the helpers convert, sort and unique the lists of the later frames
    //     (30-35 us each at 2k templates) while the caller's thread does the first one; the later collects only hand their lists over.
    // A helper spins for ~0.3 ms after a job (a stream hands them one every few tens of us) and sleeps on the condition variable otherwise.
    struct HostPool {
        std::vector<std::thread> th;
        std::mutex mu;
        std::condition_variable cv;
        std::deque<std::function<void()>> jobs;
        std::atomic<int> posted{0};                 // jobs in the queue
        std::atomic<int> asleep{0};                 // helpers waiting on cv
        bool stop = false, started = false;
        int threads = 3;
    } pool;
    // host-side wall time of the streamed path, accumulated (lm_detector_host_profile): [0] frames, [1] staging copy, [2] H2D enqueue,
    // [3] slot bookkeeping, [4] batch launches, [5] collect: waiting for the GPU, [6] record conversion, [7] canonical sort + unique
    double host_prof[8] = {};
    uint64_t ncand_hint = 0;                        // coarse candidates of the last collected frame: sizes k_dedupe's grid
    bool async_collect = true;                      // lm_detector_set_async_collect / LM_ASYNC_COLLECT=0: the lists of a batch's later frames are prepared by the helper threads

    // Live-stream ingest (lm_detector_submit_frame): one ring entry per result slot.  The host frame is staged in the entry's
    // pinned buffer (or written there by the caller: lm_detector_ingest_buffer), copied to the entry's device buffers on a
    // dedicated copy stream — the H2D of frame k+1 runs beside the front end of frame k and the matching kernels of k-1 —
    // and the front end reads it there.  An entry is free again when its frame was collected.
    struct Ingest {
        PinBuf<uint8_t> pinned[kSlots];
        DevBuf<uint8_t> d_rgb[kSlots];                 // colour image, then (16-byte aligned) the depth image: ONE upload per frame, the pinned entry has the same layout
        uint16_t* d_depth[kSlots] = {};                // = d_rgb + depth_off
        size_t depth_off = 0;
        size_t src_depth_off = 0;                      // the same in an entry of the source size (the pinned entry and d_src; == depth_off for an aligned source)
        DevBuf<uint8_t> d_src[kSlots];                 // the frame at its source size, where that is not aligned: the upload goes here and k_frame_border writes d_rgb / d_depth
        DevEvent t0[kSlots], t1[kSlots];               // timing of the H2D (copy stream); created with ingest_stream
        bool used[kSlots] = {};                        // the slot's frame came in through the ring (lm_timings.h2d_ms from t0/t1)
        hipEvent_t reader[kSlots] = {};                // front end (of another slot: a resident re-match of the streamed frame) that still reads the entry (not owned: a slot's fe_done)
    } ingest;

    // multi-GPU exchange on the device (exchange.cpp): its own stream (xchg_stream), so that the sort of frame k's records, the caller's
    // RCCL all-gather and the merge run beside the matching kernels of frame k+1
    struct Exchange {
        DevBuf<int32_t> d_merged[kSlots];
        DevBuf<ulonglong2> d_runs;                  // scratch of the per-rank sort
        PinBuf<int32_t> h_merged[kSlots];
        DevEvent done[kSlots];                      // created by the first exchange (ensure_exchange)
        int state[kSlots] = {};                     // 0 idle, 1 packed, 2 merged (result on its way to h_merged)
        int cap[kSlots] = {}, world[kSlots] = {};
        int done_slot[kSlots] = {};                 // the slot whose `done` event covers this frame's group
    } xchg;
    int local_blocks = 0;
    int num_cus = 256;

    // template extraction on the device (train.hip): scratch of the view being prepared + per-view candidate lists of a chunk
    struct Train {
        DevBuf<uint8_t> mask[kMaxLevels], lab[kMaxLevels], user_mask;
        DevBuf<int32_t> hrun[kMaxLevels];
        DevBuf<unsigned long long> keys;
        DevBuf<uint32_t> counts;
        DevBuf<int32_t> bbox, out;
    } train;
    int64_t train_stats[4] = {};     // views since creation / read(): selected on the device, sent to the host selection, failed (-1), empty (lm_detector_train_stats)

    lm_timings timings{};
};


// detector.cpp
int lm_need_both(const lm_detector* d, const char* what);   // LM_OK for the default set, else LM_ERR_INVALID "<what> needs both modalities"
extern const char* const kModalityName[2];                  // "ColorGradient", "DepthNormal"

// detector_frame.cpp
int border_resolve(const lm_detector* d, int W, int H, int* Wa, int* Ha);   // the aligned size of a W x H source under the detector's policy (strict: W x H, whatever it is)
int setup_geometry(lm_detector* d, int W, int H, bool check_match_preconditions);
int upload_frame(lm_detector* d, const uint8_t* rgb, const uint16_t* depth, int W, int H, const uint8_t* const* masks, bool check_match_preconditions);
int run_frontend_training(lm_detector* d);

// detector_bank.cpp
int upload_bank(lm_detector* d);
int lm_parts_refused(const lm_detector* d, const char* what);   // LM_OK while part matching is off, else LM_ERR_INVALID "<what> is not available under part matching"
int build_work(lm_detector* d, const char* const* class_ids, int num_class_ids);

// What the units of the streamed path share among themselves (hidden: the library's dynamic symbols stay what they were).
#pragma GCC visibility push(hidden)
// detector_frontend.cpp.  stages: bit 0 = quantise, bit 1 = the response memories (a slab pass of lm_detector_match_slabs runs 2 alone: the maps do not depend on masks).
enum { kFeQuantise = 1, kFeMemories = 2 };
int run_frontend_batch(lm_detector* d, int first, int nb, hipStream_t s, bool direct_low, bool direct_top, int stages = kFeQuantise | kFeMemories);
int lm_need_resident(const lm_detector* d, bool nothing_in_flight);                     // LM_OK, or LM_ERR_INVALID "no frame resident ..." / "frames in flight: collect them first"
// detector_launch.cpp
int slot_begin(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids, const uint8_t* rgb, const uint16_t* depth,
               const bool have_mask[2], int ring);                                      // the next result slot for a frame; nothing is launched
#pragma GCC visibility pop

// detector_frontend.cpp
int lm_quantise_resident(lm_detector* d);                                               // the quantising stages of the resident frame alone, on `stream` (depth slabs)
// the whole front end of the resident frame with BYTE linear memories at every level, on `stream`; *arena = the set written (depth-scaled matching)
int lm_byte_memories_resident(lm_detector* d, int* arena);

// detector_launch.cpp
int lm_submit_frame(lm_detector* d, float threshold, const char* const* class_ids, int num_class_ids);
int lm_launch_pending(lm_detector* d);                                                  // launches the frames waiting for their batch to fill

// detector_collect.cpp
int lm_collect_frame(lm_detector* d, int sort_unique, lm_match** out, size_t* n_out);   // sort_unique < 0: discard the records

// The host clock of the streamed path (steady_clock): seconds from a to b, and seconds since the clock's epoch — what the launch-timing model counts in.
static inline double seconds_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
static inline double host_seconds(std::chrono::steady_clock::time_point t) { return seconds_between({}, t); }

// What the launch-timing model asks of the GPU (launch_model.h): has the batch launched from leader slot `slot` finished?
struct BatchEvents {
    lm_detector* d;
    bool finished(int slot) const { return hipEventQuery(d->slot[slot].done) == hipSuccess; }
    void queries_end() const { (void)hipGetLastError(); }                               // hipErrorNotReady is not an error
};
static_assert(LaunchModel::kMaxFrames == kMaxBatch, "the launch-timing model keeps a measured time per batch size");

// host_pool.cpp: the helper threads of the streamed path (HostPool above) and the staging copy they share with the caller
bool pool_ready(lm_detector* d);
bool pool_run_one(lm_detector* d);
void pool_post(lm_detector* d, std::function<void()> job);
void pool_stop(lm_detector* d);
void staged_copy(lm_detector* d, uint8_t* dst, const uint8_t* a, size_t na, uint8_t* dst_b, const uint8_t* b, size_t nb);

// match_lists.cpp
struct ListClock { std::chrono::steady_clock::time_point converted, merged; };   // a result list: records converted, list sorted + uniqued
size_t merge_matches_impl(lm_match* m, size_t n, bool distinct_input);
lm_match* reference_order_list(const Candidate* recs, const Candidate* coarse, uint64_t ncand, size_t alive, const std::vector<int32_t>& wcls,
                               const std::vector<int32_t>& wtid, size_t* n_out, ListClock* clock);

// A writer on the frame stream (`stream`) — upload, frame selection with a geometry change, training — touches level buffers, arenas and the
// resident frame that a batch in flight on the matching stream reads.  Stream order only runs the other way (order_after_default_stream: batch
// after `stream`), so these entry points must find nothing launched and uncollected; they check it at run time and refuse.  A DIAG build
// (make DIAG=1) also aborts loudly if a future writer forgets the check.
#ifdef LM_DIAG
#include <stdio.h>
#include <stdlib.h>
struct LaunchClock {                                          // LM_LAUNCH_PROF: host time of the steps of a batch launch and of individual HIP calls in them; LM_LAUNCH_SERIES: the first 80 of each, one by one
    const char* name; double t0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    explicit LaunchClock(const char* n) : name(n), t0(now()) {}
    ~LaunchClock() {
        static std::map<std::string, std::pair<double, long>> acc;
        const double dt = now() - t0;
        auto& a = acc[name]; a.first += dt; ++a.second;
        if (getenv("LM_LAUNCH_SERIES") && a.second <= 80) fprintf(stderr, "  %s #%ld: %.0f us\n", name, a.second, 1e6 * dt);
        if (getenv("LM_LAUNCH_PROF") && a.second % 64 == 0) fprintf(stderr, "  call %-22s %.1f us (n=%ld)\n", name, 1e6 * a.first / a.second, a.second);
    }
};
#define LM_CLOCK(n) LaunchClock lm_clock_##__LINE__(n)
#define LM_DIAG_IDLE(d, what)                                                                                                    \
    do {                                                                                                                         \
        if ((d)->n_launched != (d)->n_collected) {                                                                               \
            fprintf(stderr, "LM_DIAG: %s writes on the frame stream with %llu batches' frames launched and %llu collected\n", (what), \
                    (unsigned long long)(d)->n_launched, (unsigned long long)(d)->n_collected);                                 \
            abort();                                                                                                             \
        }                                                                                                                        \
    } while (0)
#else
#define LM_CLOCK(n)
#define LM_DIAG_IDLE(d, what) do { } while (0)
#endif
