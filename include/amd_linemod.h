/*
 * amd_linemod.h — C ABI of libamdlinemod.so, the MI355X (gfx950) implementation of the
 * linemodLevelup hot path (LINE-MOD template matching + point-to-plane ICP pose refinement).
 *
 * This is the drop-in boundary for the reference's pybind11 module `linemodLevelup_pybind`
 * (/root/reference/linemodLevelup/pybind11.cpp:7-35).  Every entry point below names the reference
 * interface it replaces ("pybind11.cpp:N" = binding, "LL.cpp:N"/"LL.h:N" = linemodLevelup.{cpp,h}).
 * Plain pointers and sizes only; no torch / OpenCV / STL types.  The Python wrapper
 * 6dpose_amd/linemodLevelup_pybind.py and bench.py are the only intended callers; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every `int` function returns LM_OK (0) or a negative LM_ERR_* code unless stated otherwise;
 *     lm_last_error() returns a thread-local message (the reference raises cv::Exception ->
 *     Python RuntimeError for the same preconditions, e.g. LL.cpp:1136,1217-1218,1291,1707).
 *   - images are C-contiguous host buffers borrowed for the duration of the call:
 *     rgb  uint8  [height][width][3]  (channel order as given, LL.cpp:391-412 is order-sensitive)
 *     depth uint16 [height][width]    (millimetres)
 *     mask uint8  [height][width]     (non-zero = valid), may be NULL
 *   - a detector owns one HIP stream on one device; handles are not re-entrant.
 *   - there is NO CPU fallback: creation fails (LM_ERR_NO_DEVICE) when no gfx950 device is visible.
 */
#ifndef AMD_LINEMOD_H
#define AMD_LINEMOD_H

#include <stddef.h>
#include <stdint.h>

#include "amd_linemod_depth.h"   /* lm_depth_mode_options, lm_depth_mode, lm_slab */
#include "amd_linemod_pso.h"     /* lm_pso_options, lm_pso_result */
#include "amd_linemod_scaled.h"  /* lm_scaled_match, lm_scaled_options */

#ifdef __cplusplus
extern "C" {
#endif

#define LM_OK 0
#define LM_ERR_INVALID (-2)     /* bad argument / violated reference precondition (CV_Assert) */
#define LM_ERR_NO_DEVICE (-3)   /* no HIP device / HIP runtime failure at creation */
#define LM_ERR_HIP (-4)         /* HIP runtime error during a call */
#define LM_ERR_IO (-5)          /* file could not be read / written / parsed */
#define LM_ERR_NOT_FOUND (-6)   /* unknown class id */
#define LM_ERR_OVERFLOW (-7)    /* pipelined mode only: candidate buffer overflow, capacity raised, resubmit the frame */

typedef struct lm_detector lm_detector;

/* linemodLevelup::Match (LL.h:225-258; bound at pybind11.cpp:16-22).  class_index indexes the
 * class list the match call used (caller's class_ids order, or sorted class order when empty). */
typedef struct lm_match {
    int32_t x;
    int32_t y;
    float similarity;
    int32_t class_index;
    int32_t template_id;
} lm_match;

/* Per-stage device time of the last match call, HIP events on the detector's stream (ms). */
typedef struct lm_timings {
    float h2d_ms;        /* frame upload (0 when the frame was already resident)            */
    float frontend_ms;   /* quantise + spread + response + linearise, all levels (A1-A7)     */
    float coarse_ms;     /* similarity over all positions at the top level + threshold (A8-A10) */
    float local_ms;      /* 16x16 refinement down the pyramid (A11)                          */
    float d2h_ms;        /* match download                                                   */
    float total_ms;      /* first event to last event                                        */
    int64_t coarse_candidates;
    int64_t local_evals;
    int64_t matches_pre_unique;
    int64_t templates;   /* template pyramids searched by this rank                          */
    int64_t coarse_bytes;/* algorithmic response bytes read by the coarse pass  */
    int64_t local_bytes; /* algorithmic response bytes read by the local pass                */
    float host_submit_ms;  /* host wall time: call entry -> everything enqueued               */
    float host_wait_ms;    /* host wall time blocked in the stream synchronisation            */
    float host_collect_ms; /* host wall time: read-back bookkeeping + record conversion       */
    float host_merge_ms;   /* host wall time: canonical sort + unique (0 when not requested)  */
    int32_t batch_frames;  /* frames served by the launches the stage times above belong to (1 for a lone frame;
                            * lm_detector_submit_frame batches): per-frame device time = stage time / batch_frames */
} lm_timings;

const char *lm_last_error(void);
const char *lm_version(void);
/* Number of visible HIP devices (0 when none / runtime unavailable). */
int lm_device_count(void);
/* Binds the CALLING THREAD (and the threads it starts afterwards) to the CPUs local to `device` (sysfs local_cpulist of its PCI
 * function), within what the thread was allowed before; cpulist_out (optional) receives the list.  Call it before creating the
 * detector: the pinned staging buffers of lm_detector_submit_frame then live on the GPU's NUMA node.  A deployment that already
 * runs under numactl / a cpuset needs nothing.  No reference counterpart (the reference has no device). */
int lm_bind_thread_near_device(int device, char *cpulist_out, size_t cap);

/* ---- Detector -------------------------------------------------------------------------------
 * Detector(), Detector(T), Detector(num_features, T): pybind11.cpp:26-28, LL.cpp:1663-1692.
 * num_features <= 0 selects the default 63; T==NULL selects {5,8}.  `device` is the HIP ordinal. */
int lm_detector_create(int num_features, const int *T, int num_levels, int device, lm_detector **out);
/* The modality set: Detector(const std::vector<Ptr<Modality>>&, const std::vector<int>& T), LL.cpp:1694-1700.  `modalities` names the
 * set as the class YAML does: {"ColorGradient", "DepthNormal"} (what lm_detector_create builds; modalities == NULL selects it too),
 * {"ColorGradient"} or {"DepthNormal"}; any other list (unknown name, duplicate, the pair reversed) is LM_ERR_INVALID.  The parameters
 * are those of the reference's own constructors (LL.cpp:1684-1692): ColorGradient(10, num_features, 55), DepthNormal(2000, 50,
 * num_features, 2).  The set is fixed for the detector's life.  With ONE modality:
 *   - every call that takes the two sources (lm_detector_match, _set_frame, _store_frame, _submit_frame, _add_template) takes NULL for
 *     the absent one (a non-NULL pointer there is LM_ERR_INVALID, as NULL for a present source always was); nothing of the absent
 *     image is uploaded, quantised or written.  lm_detector_ingest_buffer returns NULL for it.
 *   - `masks`, where a call takes them, has one entry: masks[0] belongs to the set's modality.
 *   - a template pyramid has `levels` templates (not levels * 2): lm_detector_get_template's index, lm_detector_add_class_packed's arrays,
 *     class files (`modalities: [ ColorGradient ]`) and the packed bank follow; the score is raw * 100 / (4 * features of that modality),
 *     cropTemplates takes its box over that modality's features, and lm_detector_add_template returns -1 by that modality alone.
 *   - lm_detector_read_class / _read_bank / _read_params refuse a file written for another set (LL.cpp:2047-2051), in both directions.
 *   - lm_detector_read_stage refuses the absent modality's kinds; kind 4 returns the one block.
 *   - lm_pipeline_create, lm_detector_set_shard and the exchange calls return LM_ERR_INVALID ("... needs both modalities").
 * lm_detector_get_modalities returns the number of modalities (0 for a NULL detector) and, when `names` is given, static strings. */
int lm_detector_create_modalities(int num_features, const int *T, int num_levels, int device, const char *const *modalities,
                                  int num_modalities, lm_detector **out);
int lm_detector_get_modalities(const lm_detector *d, const char *names[2]);
/* The colour image's format: 3 interleaved channels (the default) or 1, a grey image (a mono8 camera).  Set once, after creation: anything but
 * 1 or 3 is LM_ERR_INVALID, as are 1 on a detector without the colour modality and a change with frames in flight.  Every entry point that takes
 * a colour pointer (lm_detector_match, _set_frame, _store_frame / _select_frame, _submit_frame, _ingest_buffer, _add_template) then reads or
 * returns width * height * channels bytes; no signature changes.  A grey frame g gives at every pyramid level, byte for byte, what the three-channel
 * frame with R = G = B = g gives (quantizedOrientations takes channel 0 where the three magnitudes are equal, LL.cpp:395-412; cv::pyrDown keeps
 * equal channels equal) — by kernels that load, stage, blur and differentiate one channel.  A change drops the resident frame and the frames parked
 * by lm_detector_store_frame.  The setting is state of this detector in this process: class files, packed banks and lm_detector_write_params do not store it,
 * and templates are the same objects either way — a bank trained in grey loads into an RGB detector and the other way round.
 * lm_detector_add_templates_rendered on a grey detector converts the rasteriser's colour image with lm_rgb_to_grey's arithmetic, on the device. */
int lm_detector_set_colour_channels(lm_detector *d, int channels);
int lm_detector_get_colour_channels(const lm_detector *d);
/* Frames of any size.  The reference asserts (src.rows * src.cols) % 16 == 0 (LL.cpp:1136) and response_map.rows / cols % T == 0 at every
 * pyramid level (LL.cpp:1217-1218); the border policy says what the MATCHING entry points (lm_detector_match, _set_frame, _store_frame,
 * _submit_frame, _ingest_buffer, lm_pipeline_create / _set_views) do with a width x height that breaks them:
 *   0 strict (the default): refused with LM_ERR_INVALID and the assert's words, as the reference does;
 *   1 pad:   the frame is extended at the right and bottom to the aligned size — colour / grey by edge replication (what the reference's
 *            BORDER_REPLICATE stages assume at a frame edge: no gradient appears), depth and every mask with 0 (no measurement: no normals);
 *   2 crop:  the frame is cut at the right and bottom to the aligned size.
 * The source's top-left pixel stays at (0, 0), so match coordinates, K and principal points keep their meaning.  Every entry point then
 * returns bit for bit what the strict policy returns for the frame padded that way, or for frame[:Ha, :Wa], on the host; matches whose box
 * reaches into the padded margin are kept (they are records of the padded frame).  The caller hands over — and the pinned staging holds,
 * and PCIe carries — the SOURCE size: rgb, depth, masks and lm_detector_ingest_buffer's pointers are width x height.  The frame buffers, the
 * frames parked by lm_detector_store_frame and lm_detector_read_stage have the ALIGNED size; a kernel on the device (k_frame_border) writes them.
 * A size that is aligned already takes the strict path unchanged.  Training (lm_detector_add_template, _add_templates_rendered) takes any
 * size under every policy.  A change is LM_ERR_INVALID with frames in flight.
 * The aligned size, for pad: the smallest Ha >= height, then the smallest Wa >= width, for crop the largest Ha <= height, then the largest
 * Wa <= width (both at least 16, else LM_ERR_INVALID "unsupported frame size"), such that at every level l of the L levels
 * (Wa >> l) % T[l] == 0, (Ha >> l) % T[l] == 0, Wa and Ha are multiples of 2^(L-1), and ((Wa >> l) * (Ha >> l)) % 16 == 0.
 * lm_detector_aligned_size answers for `policy` (-1: the detector's own); under 0 it returns the size itself or the strict refusal. */
int lm_detector_set_border(lm_detector *d, int policy);
int lm_detector_get_border(const lm_detector *d);
int lm_detector_aligned_size(const lm_detector *d, int policy, int width, int height, int *aligned_width, int *aligned_height);
/* grey[i] = (4899 R + 9617 G + 1868 B + 8192) >> 14 for the `pixels` pixels of an interleaved R, G, B image, on `device`: the 8-bit fixed point of
 * OpenCV's RGB2GRAY (unpinned: not checked against an OpenCV build).  For training a grey detector from colour photographs. */
int lm_rgb_to_grey(int device, const uint8_t *rgb, int64_t pixels, uint8_t *grey);
void lm_detector_destroy(lm_detector *d);

/* Detector::addTemplate (pybind11.cpp:29, LL.cpp:1943-1975).  Returns the new template_id (>=0),
 * -1 when no valid template could be extracted (the reference's own convention, LL.cpp:1964-1966),
 * or an LM_ERR_* code (< -1).  Quantisation runs on the GPU; so does the greedy feature selection when a mask is given
 * (train.hip, checked against the reference's golden YAML), on the host for the maskless call. */
int lm_detector_add_template(lm_detector *d, const uint8_t *rgb, const uint16_t *depth, const uint8_t *mask,
                             int width, int height, const char *class_id);

/* Detector::readClasses / writeClasses for ONE class (pybind11.cpp:30-31; LL.cpp:2043-2146):
 * OpenCV FileStorage YAML 1.0 schema; `.gz` paths are NOT supported by this library (the Python
 * wrapper decompresses).  read returns LM_ERR_INVALID on the reference's CV_Asserts (modalities,
 * pyramid_levels, consecutive template ids, class already present). */
int lm_detector_read_class(lm_detector *d, const char *path, const char *class_id_override);
int lm_detector_write_class(lm_detector *d, const char *class_id, const char *path);

/* Detector::write / Detector::read (LL.cpp:2013-2041; C++-only in the reference): pyramid_levels, T and the parameters of
 * the two modalities (ColorGradient::write :686-692, DepthNormal::write :1012-1020) as OpenCV FileStorage YAML.  read clears
 * the classes (LL.cpp:2015). */
int lm_detector_write_params(const lm_detector *d, const char *path);
int lm_detector_read_params(lm_detector *d, const char *path);

/* Bulk import of a packed class (binary bank for >=16k templates).
 * features: [total][3] int32 (x,y,label); tmpl_offsets: [num_pyramids*levels*2+1] prefix offsets in
 * reference TemplatePyramid order (level-major, modality-minor; LL.h:336-337); tmpl_wh:
 * [num_pyramids*levels*2][2] width,height. */
int lm_detector_add_class_packed(lm_detector *d, const char *class_id, int num_pyramids,
                                 const int32_t *features, const int32_t *tmpl_offsets, const int32_t *tmpl_wh);

/* Packed binary bank file next to the reference's one-YAML-per-class files (LL.cpp:2124-2146): the same
 * information — class id, per template width/height/pyramid level, per feature x, y, label (LL.cpp:2072-2122) — as flat
 * arrays, 4 bytes per feature (x int16, y int13, label 3 bits), read through mmap.  write: the named classes, or all of
 * them when num_class_ids == 0; LM_ERR_INVALID when a feature does not fit the packing (the YAML path has no such
 * limit).  read: adds the named classes of the file (all when num_class_ids == 0), so a rank that serves some of the
 * objects touches only their part of the file; pyramid_levels must match (LL.cpp:2052), a class already present is an
 * error (LL.cpp:2059) and then nothing is added.  lm_bank_file_info / _class_id inspect a file without a detector. */
int lm_detector_write_bank(const lm_detector *d, const char *path, const char *const *class_ids, int num_class_ids);
int lm_detector_read_bank(lm_detector *d, const char *path, const char *const *class_ids, int num_class_ids);
int lm_bank_file_info(const char *path, int32_t *pyramid_levels, int32_t *num_classes, int64_t *num_pyramids, int64_t *num_features);
int lm_bank_file_class_id(const char *path, int index, char *out, int capacity);
/* The modality set a bank file was written for: returns the count (1 or 2; < 0 = LM_ERR_*) and the names as static strings.  The set
 * lives in a header word that was reserved (zero) before: every older file reads as [ColorGradient, DepthNormal].  lm_detector_read_bank
 * refuses a file whose set differs from the detector's. */
int lm_bank_file_modalities(const char *path, const char *names[2]);

/* Detector::numClasses / classIds / numTemplates (LL.h:343, LL.cpp:1984-2011). */
int lm_detector_num_classes(const lm_detector *d);
const char *lm_detector_class_id(const lm_detector *d, int index);   /* sorted (std::map) order */
int lm_detector_num_templates(const lm_detector *d, const char *class_id); /* NULL = all classes */
int lm_detector_pyramid_levels(const lm_detector *d);
int lm_detector_get_T(const lm_detector *d, int level);

/* Detector::getTemplates (pybind11.cpp:34, LL.cpp:1976-1982): entry `index` (0..levels*2-1) of
 * template pyramid `template_id`.  Writes width/height/pyramid_level/num_features; copies at most
 * `capacity` features (x,y,label triples) into `features` (may be NULL to query the count). */
int lm_detector_get_template(const lm_detector *d, const char *class_id, int template_id, int index,
                             int32_t *width, int32_t *height, int32_t *pyramid_level,
                             int32_t *num_features, int32_t *features, int capacity);

/* Multi-GPU sharding: this rank searches the contiguous slice
 * [N*rank/world, N*(rank+1)/world) of the N template pyramids a match call selects; template ids
 * stay global.  Default (0,1). */
int lm_detector_set_shard(lm_detector *d, int rank, int world);

/* Multi-GPU exchange on the device.  Detector::match sorts and adjacent-uniques the records of ALL templates
 * (LL.cpp:1771-1776); with the bank sharded over W ranks that is a distributed merge sort, done without the host:
 *   lm_detector_submit(...)                         this rank's shard of the frame
 *   lm_detector_exchange_pack(d, send, capacity)    sorts the rank's distinct records into `send` (device memory,
 *                                                   lm_exchange_block_bytes(capacity) bytes: header + a sorted run of keys)
 *   all-gather of the W blocks into `recv`          the caller's collective (RCCL), enqueued on lm_detector_exchange_stream(d)
 *   lm_detector_exchange_merge(d, recv, W, capacity) merges the W runs, marks what std::unique drops, copies to pinned memory
 *   lm_detector_exchange_collect(d, &out, &n, &failed) waits for the oldest frame in flight: the same list on every rank,
 *                                                   identical to an unsharded lm_detector_match (lm_free(out))
 * pack / merge apply to the most recently submitted frame and only enqueue work on the exchange stream (hipStream_t
 * returned as void*); up to lm_detector_max_in_flight() frames can be in flight.  capacity: power of two in [256, lm_exchange_max_capacity()] (65536), the same on every rank.
 * *failed != 0 (on every rank alike, *out == NULL): > 0 some rank had that many distinct records (> capacity), < 0 a
 * candidate buffer overflowed or a field did not fit the key — rerun the frame through lm_detector_match_resident +
 * lm_merge_matches (sharded.py does). */
int lm_exchange_max_capacity(void);
int lm_detector_max_in_flight(void);
void *lm_detector_exchange_stream(lm_detector *d);
size_t lm_exchange_block_bytes(int capacity);
int lm_detector_exchange_pack(lm_detector *d, void *send_block, int capacity);
int lm_detector_exchange_merge(lm_detector *d, const void *recv_blocks, int world, int capacity);
/* The same for a frame named by its number in submission order (0, 1, ...): a streamed frame is launched with its batch, so its
 * exchange is enqueued once lm_detector_frames_launched() has passed it (sharded.DeviceExchange does this for every frame, in
 * order, after each submit and before each collect).  frames_submitted() is the number the next submitted frame gets. */
uint64_t lm_detector_frames_submitted(const lm_detector *d);
uint64_t lm_detector_frames_launched(const lm_detector *d);
uint64_t lm_detector_frames_collected(const lm_detector *d);
int lm_detector_exchange_pack_frame(lm_detector *d, uint64_t frame_no, void *send_block, int capacity);
int lm_detector_exchange_merge_frame(lm_detector *d, uint64_t frame_no, const void *recv_blocks, int world, int capacity);
/* One all-gather for a GROUP of frames: every rank sends [frame][block] and receives [rank][frame][block]; recv_blocks = this frame's
 * block of rank 0, rank j's lies j * rank_stride_bytes further. */
int lm_detector_exchange_merge_frame_strided(lm_detector *d, uint64_t frame_no, const void *recv_blocks, int world, int capacity,
                                             size_t rank_stride_bytes);
/* ... and the n frames of a group in one call: frame first + i uses block i of send_blocks / of every rank's part of recv_blocks. */
int lm_detector_exchange_pack_group(lm_detector *d, uint64_t first, int n, void *send_blocks, int capacity);
int lm_detector_exchange_merge_group(lm_detector *d, uint64_t first, int n, const void *recv_blocks, int world, int capacity);
int lm_detector_exchange_collect(lm_detector *d, lm_match **out, size_t *n, int *failed);
/* the same into caller memory (capacity records; world * capacity always suffices): no allocation, one pass */
int lm_detector_exchange_collect_into(lm_detector *d, lm_match *dst, size_t capacity, size_t *n, int *failed);

/* The collective, issued by the library (BASELINE north_star: "RCCL all-gather over xGMI of per-GPU top-K matches"; the caller shape is the
 * reference's C++ driver, linemodLevelup/test.cpp:111-130, one process per GPU).  librccl.so is loaded at run time (dlopen; LM_RCCL_LIB
 * names another file), so single-GPU use needs no RCCL.  Rank 0 calls lm_comm_unique_id and carries the 128 bytes to the other ranks by
 * whatever it has (MPI_Bcast, a file, a socket, torch.distributed's store): the library has no transport of its own.
 *   lm_comm_available()                                1 if librccl.so could be loaded
 *   lm_comm_create(id, rank, world, device, &comm)     ncclCommInitRank on this rank's device (collective: every rank calls it)
 *   lm_exchange_allgather(d, comm, send, recv, bytes)  ncclAllGather of `bytes` per rank on lm_detector_exchange_stream(d): in stream order
 *                                                      after the pack kernels of the frames it carries, before their merges; nothing blocks the host
 *   lm_detector_exchange_group(d, comm, first, n, send, recv, capacity)
 *                                                      pack_group + all-gather + merge_group of frames first .. first + n - 1 in one call
 *                                                      (send: n blocks, recv: world x n blocks of lm_exchange_block_bytes(capacity), device memory) */
typedef struct lm_comm lm_comm;
int lm_comm_available(void);
int lm_comm_unique_id(void *id128);
int lm_comm_create(const void *id128, int rank, int world, int device, lm_comm **out);
void lm_comm_destroy(lm_comm *c);
int lm_comm_rank(const lm_comm *c);
int lm_comm_world(const lm_comm *c);
int lm_exchange_allgather(lm_detector *d, lm_comm *c, const void *send, void *recv, size_t bytes_per_rank);
int lm_detector_exchange_group(lm_detector *d, lm_comm *c, uint64_t first, int n, void *send_blocks, void *recv_blocks, int capacity);

/* Detector::match (pybind11.cpp:32-33, LL.cpp:1702-1777).  class_ids may be NULL/0 = all classes.
 * masks: NULL, or two pointers (colour, depth modality), each NULL or a [height][width] uint8 mask.
 * On success *out is a malloc'd array of *n matches in the canonical order of SURVEY §8a A12
 * (similarity desc, template_id asc, class position asc, y asc, x asc; then adjacent-unique on
 * (x,y,similarity,class)), to be released with lm_free().  With world>1 the result holds only
 * this rank's matches, still sorted+uniqued; lm_merge_matches() merges gathered lists. */
int lm_detector_match(lm_detector *d, const uint8_t *rgb, const uint16_t *depth, int width, int height,
                      float threshold, const char *const *class_ids, int num_class_ids,
                      const uint8_t *const *masks, lm_match **out, size_t *n);

/* The same in two steps, so that a benchmark can time the device path with the frame already
 * resident in HBM: lm_detector_set_frame uploads (and keeps) the frame; lm_detector_match_resident
 * runs front end + matching on it.  `sort_unique`: 1 = canonical sort + unique (Detector::match); 0 = the raw pre-unique
 * records, unordered; 2 = the records without exact duplicates (same x, y, template: several coarse candidates refined to
 * one position; removed on the device, std::unique drops them in any merge), unordered — what the multi-GPU gather ships. */
int lm_detector_set_frame(lm_detector *d, const uint8_t *rgb, const uint16_t *depth, int width, int height,
                          const uint8_t *const *masks);
/* Stream support: park frames in HBM slots once, then make one current with a
 * device-to-device copy on the detector's stream (no host traffic inside a timed region). */
int lm_detector_store_frame(lm_detector *d, int slot, const uint8_t *rgb, const uint16_t *depth, int width, int height);
int lm_detector_select_frame(lm_detector *d, int slot);
int lm_detector_match_resident(lm_detector *d, float threshold, const char *const *class_ids, int num_class_ids,
                               int sort_unique, lm_match **out, size_t *n);
/* Pipelined stream mode: lm_detector_submit enqueues front end + matching of the current
 * frame and returns; lm_detector_collect waits for the OLDEST submitted frame and returns its matches.
 * Up to lm_detector_max_in_flight() (sixteen) frames may be in flight: the front end of frame k+2 and the matching kernels of frame k+1 run on two
 * streams while the host sorts frame k:
 *   select_frame(k+2); submit(); collect() -> frame k; ...
 * lm_detector_match_resident == submit + collect. */
int lm_detector_submit(lm_detector *d, float threshold, const char *const *class_ids, int num_class_ids);
int lm_detector_collect(lm_detector *d, int sort_unique, lm_match **out, size_t *n);
/* sort_unique = 3 (collect, match_resident), or lm_detector_set_reference_order(d, 1) for every sort_unique = 1 call of this
 * detector (lm_detector_match included; LM_REFERENCE_ORDER=1 sets it at creation): the list exactly as the reference's
 * Detector::match returns it — its std::sort (Match::operator<, which ignores x, y) and std::unique (operator==, which ignores
 * template_id) replayed on the pre-unique records in the order the reference appends them (LL.cpp:1753-1776), with the same
 * libstdc++ introsort.  Unlike the canonical order (the default) this keeps the duplicates the reference keeps: on fixture
 * bank 63 at threshold 55 it returns the reference's 560 entries, the canonical order 366 (the same 358 distinct positions).
 * Host-side cost: one extra device-to-host copy of the candidate buffer and a sort of all pre-unique records; single GPU only
 * (a sharded match merges canonically). */
int lm_detector_set_reference_order(lm_detector *d, int on);
/* Live-stream ingest (the per-frame call of linemod_ros/detect.py:83-138 and of the dataset loop
 * linemod_and_levelup_test.py:314-327, which hand a NEW host frame to every Detector.match): lm_detector_submit_frame =
 * "upload this host frame + lm_detector_submit" without blocking.  The frame is staged in a ring of pinned buffers (one per
 * frame in flight), copied to HBM on a dedicated copy stream — the H2D of frame k+1 overlaps the front end of frame k and
 * the matching kernels of frame k-1 — and the call returns as soon as everything is enqueued; rgb / depth are borrowed
 * only until it returns.  Results come back through lm_detector_collect in submission order:
 *   submit_frame(f0); submit_frame(f1); submit_frame(f2); collect() -> f0; submit_frame(f3); collect() -> f1; ...
 * Zero-copy variant: lm_detector_ingest_buffer returns the pinned staging pointers the NEXT lm_detector_submit_frame will
 * use (a camera driver / decoder writes the frame there); passing exactly these pointers skips the staging copy.
 * No masks (the reference's callers pass masks=[]).  The frame size may change only with no frame in flight
 * (LM_ERR_INVALID otherwise).  After LM_ERR_OVERFLOW from collect, submit that frame again.
 *
 * Frames per launch: a 2k-template bank does not fill the chip, so consecutive streamed frames share their kernel launches —
 * the frame's upload starts at once, its front end / coarse pass / refinement / duplicate removal are launched together with
 * those of the following frames once lm_detector_get_batch() (default 8, LM_FRAME_BATCH, lm_detector_set_batch 1..8) frames
 * with the same threshold and class list are waiting, or when lm_detector_flush or a lm_detector_collect that needs one of them
 * is called — or at once while the GPU has fewer than lm_detector_set_batch_queue (default 2, LM_BATCH_QUEUE; 0 = always wait for
 * a full batch) launched batches still to finish: the GPU never idles waiting for a batch to fill, the first frames of a stream go
 * out alone, and batches grow to the maximum exactly when the GPU is the bottleneck.  Results are unchanged and still come back per frame, in order; lm_timings.batch_frames says how many frames the
 * reported launches served.  set_batch(1) restores one launch set per frame (lowest latency). */
int lm_detector_submit_frame(lm_detector *d, const uint8_t *rgb, const uint16_t *depth, int width, int height,
                             float threshold, const char *const *class_ids, int num_class_ids);
int lm_detector_ingest_buffer(lm_detector *d, int width, int height, uint8_t **rgb, uint16_t **depth);
int lm_detector_flush(lm_detector *d);            /* launch the streamed frames that are waiting for their batch to fill */
int lm_detector_set_batch(lm_detector *d, int frames);
int lm_detector_get_batch(const lm_detector *d);
int lm_detector_set_batch_queue(lm_detector *d, int batches);
/* Streamed frames come back in batches: when lm_detector_collect (sort_unique = 1) has seen the event of a batch, the records of ALL its
 * frames are in pinned memory, and helper threads of the library (LM_HOST_THREADS, default 3, never more than the CPUs the process may use
 * leave free, 0 = none; they make no HIP calls) prepare the Detector::match lists of the batch's later frames — record conversion, canonical
 * sort, unique — while the caller takes the first; collecting those frames then only hands the list over.  The same threads copy slices of a
 * submitted frame into the pinned staging buffer beside the caller.  On by default (LM_ASYNC_COLLECT=0 / set_async_collect(d, 0) turn the
 * list preparation off); without helpers the caller does everything itself.  Results are identical either way. */
int lm_detector_set_async_collect(lm_detector *d, int on);
/* Host-side wall time (seconds, accumulated) the library spent on streamed frames: out8 = {frames, staging copy, H2D enqueue, slot
 * bookkeeping, batch launches, collect: waiting for the GPU, record conversion, canonical sort + unique}; reset != 0 clears it. */
int lm_detector_host_profile(lm_detector *d, double *out8, int reset);
/* 1 when the local refinement (similarityLocal, LL.cpp:1366-1428) of the current bank and frame geometry runs on bit planes
 * (kernel k_local_bits, or k_local_wide under refine 3 with a table of three or four distinct non-zero values), 0 when on byte
 * planes (k_local): which kernel a profile of the match shows.  Valid after a match. */
int lm_detector_refines_on_bit_planes(const lm_detector *d);
/* Which kernels serve similarity (LL.cpp:1284-1354) and similarityLocal (LL.cpp:1366-1428).  Results never depend on it; tests and
 * measurements use it to run every path against the oracle in one process.
 *   refine: 0 = bit planes (k_local_bits; default, any pyramid with a level below the top), 1 = byte strip planes with tiles (k_local),
 *           2 = byte planes, every candidate on its own (k_local without tiles).
 *           3 = wide bit planes: what 0 is for a response table of at most two distinct non-zero values (the default among them: the same
 *           kernels, the same memory, and lm_detector_get_paths answers 0); for the other tables (4 3 2 1 0, ...) two sets of bit planes
 *           (k_local_wide), where 0 falls back to the byte kernels.  Not on a sharded detector (lm_detector_set_shard): refused.
 *   coarse: 0 = bit planes (k_coarse_bits; default, used when the refinement runs on bit planes too), 1 = byte linear memories (k_coarse),
 *           2 = wide bit planes (k_coarse_wide for the tables that need it, else what 0 is); it plans no tiles, so only with refine 3.
 * Refused with frames in flight.  lm_detector_get_paths reports what the current bank and frame geometry actually use (valid after a
 * match): refine 0 / 1 / 2 / 3 and coarse 0 / 1 / 2 as above — 3 / 2 only when the wide kernels ran.  What sends a bank or geometry off the
 * bit planes (a single-level pyramid, LM_BITPLANES=0, entries beyond 16383 features) does so under 3 / 2 as well.  The front end writes byte
 * planes for a table on the wide kernels and two kernels pack both sets from them (lm_detector_set_direct_bits has no say there). */
int lm_detector_set_paths(lm_detector *d, int refine, int coarse);
int lm_detector_get_paths(const lm_detector *d, int *refine, int *coarse);
/* The response table of computeResponseMaps: r[d] = the response to a feature whose label lies at cyclic distance d (0..4, eight orientations)
 * from the nearest orientation set in the spread image.  The reference holds five such tables (LL.cpp:1112-1124) and compiles one; here it is
 * detector state: 4 1 0 0 0 by default (LL.cpp:1121, the reference's live one), 4 3 2 1 0 is the original LINE-MOD / cv::linemod table (:1112).
 * Accepted: r[0] == 4 (the score stays raw * 100 / (4 * features), LL.cpp:1842, 1918), values non-increasing — 70 tables; anything else is
 * LM_ERR_INVALID.  Refused with frames in flight.  Every match runs the front end of its frame, so the next match — lm_detector_match_resident
 * of the frame already resident included — builds its response memories under the new table.  The table is state of this detector in this
 * process (lm_detector_read_stage: kinds 2 / 3 answer under the table in force — the byte planes are rebuilt from the last frame's quantised maps
 * when the table changed since —, kinds 4 / 5 show what the last match read): lm_detector_write_classes / lm_detector_write / the packed bank do not store it, training (lm_detector_add_template) does not read
 * it, and the ranks of a sharded run must each set the same one.  Tables with at most two distinct non-zero values (4 1 0 0 0, 4 2 0 0 0,
 * 4 1 1 0 0, ...) run on the bit-plane kernels; the others (4 3 2 1 0, 4 2 1 0 0, 4 3 1 0 0, ...) run on the byte kernels — or, when
 * lm_detector_set_paths(d, 3, 2) asked for them, on the wide bit-plane kernels —, which lm_detector_get_paths reports.  Thresholds are not comparable between tables. */
int lm_detector_set_response_table(lm_detector *d, const uint8_t r[5]);
int lm_detector_get_response_table(const lm_detector *d, uint8_t r[5]);
/* Part-based matching: accept a template when min_parts of its 4 quadrants match, the reference author's first answer to occlusion
 * (linemodLevelup/notes.md:1-9: "cut template to 4 parts ... if half of the obj is hidden, original holistic match's average response will drop
 * to 50%, while part-based match keeps 100%").  Off by default (min_parts 0); 1..4 switches it on.  The rule, per template entry (pyramid, level):
 *   a feature at (x, y) belongs to part (2 x >= width) + 2 (2 y >= height), both modalities pooled; a part of n_p features is eligible iff
 *   n_p >= min_part_features (>= 1; parts too small to mean anything never pass);
 *   top level: a position below the template's position count is a candidate iff at least min_parts eligible parts have
 *   (raw_p * 100.f) / (4 * n_p) > threshold (the expression and strict comparison of LL.cpp:1842-1844); its score is the holistic one;
 *   levels below: window, clamp, arg-max (first maximum of the holistic sum) and position update as always (LL.cpp:1871-1931); the candidate
 *   stays iff at least min_parts eligible parts have (raw_p at the arg-max position * 100.f) / (4 * n_p) >= threshold (LL.cpp:1935 drops `<`).
 * lm_match.similarity stays the HOLISTIC score at level 0, so under part matching it may lie below the threshold.  Record format, duplicate
 * removal and both result orders are unchanged; min_parts 4 is stricter than the holistic rule, 2 tolerates half the object hidden.
 * Refused (LM_ERR_INVALID), at the set or when a frame is submitted — nothing is matched holistically in silence: frames in flight at the set; a
 * threshold < 0; paths other than lm_detector_set_paths(d, 0, 0); a response table of more than two distinct non-zero values; a bank whose
 * refinement windows can leave their planes (features outside the template's box, a template wider than the frame minus 16 T); a sharded
 * detector and the multi-GPU exchange; lm_detector_match_slabs; lm_pipeline_create / lm_pipeline_run on such a detector.
 * lm_part_table is the host's part table of one entry, callable without a GPU: out16 = start[4], n[4], npad[4] (n rounded up to 8: the part's
 * slots in the part-ordered feature arrays, from start), eligible[4]; order (may be NULL; room for n + 28 entries) = per slot the index of its
 * feature, -1 for padding. */
int lm_detector_set_part_matching(lm_detector *d, int min_parts, int min_part_features);
int lm_detector_get_part_matching(const lm_detector *d, int *min_parts, int *min_part_features);
int lm_part_table(int width, int height, const int32_t *xs, const int32_t *ys, int n, int min_part_features, int32_t *out16, int32_t *order);
/* Depth slabs: template scales chosen from the scene's depth histogram (the reference's "use depth histogram and 1D nms to find some primary
 * scales", linemodLevelup/readme.md:29-34, notes.md: train each scale as a class of its own and match it only where the scene has that depth).
 *
 * lm_detector_depth_modes: the primary depths of the RESIDENT frame (lm_detector_set_frame / select_frame; the aligned geometry of
 * lm_detector_set_border, whose padding is depth 0 and counts nowhere).  Integers only, so the result is exact:
 *   nbins = ceil((far_mm - near_mm) / bin_mm); a pixel with near_mm <= d < far_mm counts in bin (d - near_mm) / bin_mm;
 *   bin b is a mode iff h[b] >= min_pixels, h[b] > h[j] for j in [b - window, b) and h[b] >= h[j] for j in (b, b + window] (bins outside
 *   [0, nbins) do not exist; on a plateau the lowest bin wins); depth_mm = near_mm + b * bin_mm + bin_mm / 2;
 *   the max_modes modes with the most pixels are returned, most pixels first, ties towards the smaller depth.
 * options NULL = the defaults of lm_depth_mode_options_init.  out has room for `capacity` >= max_modes records; *n receives the count.
 * LM_ERR_INVALID: options outside the limits stated in amd_linemod_depth.h, a detector without DepthNormal, no resident frame, frames in flight.
 *
 * lm_detector_set_class_depth_range: the band of scene depths [lo_mm, hi_mm] at which the templates of a class are valid (for a class
 * rendered at radius r, for example 0.85 r .. 1.15 r); clear != 0 removes it.  lo_mm > hi_mm is LM_ERR_INVALID, an unknown class
 * LM_ERR_NOT_FOUND.  Host state of this detector: no class file, bank file or parameter file stores it, lm_detector_read_class / _read_bank
 * produce classes without a range and lm_detector_read_params drops every range with the classes.  lm_detector_get_class_depth_range returns 1 and the range,
 * 0 when the class has none.
 *
 * lm_detector_match_slabs, on the resident frame, with modes = lm_detector_depth_modes(options):
 *   the requested classes are class_ids in their order (NULL / 0: every class, sorted); unknown names are skipped;
 *   for mode k of depth p: slab S_k = the pixels with d != 0 and p - slab_mm <= d <= p + slab_mm; classes_k = the requested classes whose
 *   range holds p.  classes_k empty: the slab is skipped (reported with no class and 0 records).  Otherwise its records are those of
 *   lm_detector_match of classes_k under the masks S_k AND the frame's own mask of each modality (lm_detector_set_frame's `masks`);
 *   the requested classes without a range are matched once under the frame's own masks only;
 *   *out = the canonical merge (lm_merge_matches) of all of it, class_index = the position in the requested list; lm_free(*out).
 * slabs[0 .. *num_slabs): one lm_slab per mode, in mode order, then one with depth_mm = -1 for the classes without a range when there are
 * any; slab_capacity >= max_modes + 1.  *slab_classes (lm_free) holds the slabs' class positions.
 * The histogram, the modes, the slab masks and their pyramid are made on the device from the resident depth image: per slab nothing crosses
 * PCIe but the records, the frame is quantised once per call, and the frame's own masks are left as they are.  Response table, paths,
 * border policy, colour_channels and a depth-only modality set apply as in lm_detector_match.  LM_ERR_INVALID: a detector without
 * DepthNormal, a sharded detector (lm_detector_set_shard), slab_mm < 0, no resident frame, frames in flight.  The streamed calls
 * (lm_detector_submit_frame) and lm_pipeline_run do not know slabs. */
void lm_depth_mode_options_init(lm_depth_mode_options *options);
int lm_detector_depth_modes(lm_detector *d, const lm_depth_mode_options *options, lm_depth_mode *out, int capacity, int *n);
int lm_detector_set_class_depth_range(lm_detector *d, const char *class_id, int lo_mm, int hi_mm, int clear);
int lm_detector_get_class_depth_range(const lm_detector *d, const char *class_id, int *lo_mm, int *hi_mm);
int lm_detector_match_slabs(lm_detector *d, float threshold, const char *const *class_ids, int num_class_ids, int slab_mm,
                            const lm_depth_mode_options *options, lm_match **out, size_t *n, lm_slab *slabs, int slab_capacity,
                            int *num_slabs, int32_t **slab_classes);
/* Depth-scaled matching: every template scaled, per matching position, to the scene depth found there (the reference author's "at each matching
 * pos, scale template depth to scene depth", linemodLevelup/notes.md:1-2, 25-31, readme.md:24: the best detector of those notes, dropped for its
 * CPU cost).  A class trained at d_train mm (lm_detector_set_class_train_depth; host state of this detector like the depth ranges, stored in no
 * file; 1..65535) is found at other distances without a class per scale: the bank is not multiplied.  The rule, on the RESIDENT frame, is the
 * holistic rule of lm_detector_match with one change, where a feature is sampled:
 *   probe map P: the smallest non-zero depth of the (2 probe + 1)^2 window of level-0 pixels around a pixel, clipped to the aligned frame; 0 if none;
 *   top level, entry (pyramid, L - 1) of box (w, h), step T, Wd = W / T: every cell (i, j) whose raster position lies below the template's
 *   position count (of the unscaled box) is looked at; d = P at the level-0 pixel ((i T + w / 2) << (L - 1), (j T + h / 2) << (L - 1)) clamped into
 *   the frame; no candidate if d = 0, d_train 1024 < min_scale_q10 d or d_train 1024 > max_scale_q10 d; else k = argmin |s_k d - d_train 1024| in
 *   64-bit integers, a tie to the lower k; k is carried through every lower level, the depth is not probed again;
 *   a feature (fx, fy) of an entry with centre c = (w / 2, h / 2) is sampled at sx = cx + sign(fx - cx) ((|fx - cx| s_k + 512) >> 10), sy alike
 *   (lm_scaled_features: the host's statement, callable without a GPU); labels, the feature count and the score's denominator stay, features
 *   that coincide after scaling count twice; its response at a position origin (ox, oy), a multiple of T, is the byte of its modality's linear
 *   memories at pixel (ox + sx, oy + sy), and 0 when that pixel's cell lies outside [0, Wd) x [0, Hd);
 *   candidates ((raw 100.f) / (4 nf) > threshold), windows, clamps (of the unscaled box), first-maximum arg-max, position updates and the drop
 *   below the threshold are those of lm_detector_match (LL.cpp:1835-1938).
 * The one DEPARTURE from the reference's reads: a cell outside the level reads 0, there is no wrap into the next row or the next linear memory
 * (with the ladder {1024} the records are those of lm_detector_match wherever no template's reads wrap).
 * Records (lm_scaled_match; lm_free(*out)): x, y, similarity of the unscaled convention, scale_index k, depth_mm d; exact duplicates removed;
 * ordered by similarity descending, then class_index, template_id, y, x, scale_index, depth_mm ascending.  options NULL = lm_scaled_options_init.
 * Candidate buffers of its own start at the detector's candidate capacity and grow (the call reruns) on an overflow: no candidate is dropped.
 * Every response table, grey colour frames, a depth-only modality set and the border policies work (the padding's depth is 0).
 * Refused (LM_ERR_INVALID), never matched unscaled in silence: a detector without DepthNormal; a sharded detector; part matching switched on;
 * a detector that serves a pipeline; frames in flight; no resident frame; a ladder that is not 1..16 strictly ascending values in [512, 2048];
 * bounds with min > max; probe outside 0..4; a requested class without a training depth; a ladder whose table (scales x the largest top-level
 * feature count x 8 bytes) exceeds 160 KB.  The call leaves no frame in flight, so the multi-GPU exchange has nothing to pack. */
void lm_scaled_options_init(lm_scaled_options *options);
int lm_detector_set_class_train_depth(lm_detector *d, const char *class_id, int depth_mm);
int lm_detector_get_class_train_depth(const lm_detector *d, const char *class_id, int *depth_mm);
int lm_detector_match_scaled(lm_detector *d, float threshold, const char *const *class_ids, int num_class_ids, const lm_scaled_options *options,
                             lm_scaled_match **out, size_t *n);
int lm_scaled_features(int width, int height, const int32_t *xs, const int32_t *ys, int n, int scale_q10, int32_t *out_xs, int32_t *out_ys);
/* Device memory ALLOCATED for the bit planes, summed over the result slots: the strip records of the levels below the top and the pair
 * stream of the top level (tests: no response table makes them grow). */
int lm_detector_bit_arena_bytes(const lm_detector *d, uint64_t *strip_records, uint64_t *pair_stream);
/* The same for the SECOND set of bit planes of the wide paths (lm_detector_set_paths 3 / 2): zero until a match has run a table of three or
 * four distinct non-zero values on them, then the sizes of the first set for every result slot that has served such a match. */
int lm_detector_wide_arena_bytes(const lm_detector *d, uint64_t *strip_records, uint64_t *pair_stream);
/* Which selection served the training views (lm_detector_add_template, lm_detector_add_templates_rendered[_ex]) since the detector was
 * created or lm_detector_read_params was called: out[0] views whose features the device selected (train.hip), out[1] views sent to the
 * host selection (LM_TRAIN_HOST=1, no or a grey object mask, more than 1024 features, a candidate list beyond what the kernel sorts),
 * out[2] views that failed with -1 (too few candidates; counted besides out[0] / out[1]), out[3] empty views (rendered views without
 * a depth pixel; neither selection ran).  Tests: a fall-back to the host selection is otherwise invisible, it gives the same templates. */
int lm_detector_train_stats(const lm_detector *d, int64_t out[4]);
/* The response maps of spread / computeResponseMaps / linearize (LL.cpp:1026-1243) as bit planes straight from the quantised images
 * (default, on = 1: wherever the kernels in use read only bit planes, the byte linear memories are not written at all) or as the
 * reference's byte linear memories first, packed into bit planes by a second kernel (on = 0).  Bit 1 (on = 2, 3): the top level's bit
 * planes stay readable after the match (lm_detector_read_stage kind 5; tests).  The top level has three writers — from pixel tiles (T = 4 or 8,
 * a multiple of 8 cells per row: whole bytes), whole dwords per wave (T * T * cells a multiple of 64), ballots OR-ed into a zeroed stream — and
 * the cheapest the geometry allows is used; bit 2 (on = 4 ...) forces the OR-ing writer, bit 3 (on = 8 ...) rules out the tiles (tests).
 * Results never depend on it. */
int lm_detector_set_direct_bits(lm_detector *d, int on);
/* The coarse pass on the pair stream has two kernels that leave the same candidates, counters and order of a template's hits inside a
 * frame: k_coarse_bits (a wave serves one template on one frame) and k_coarse_bits_batch (the frames of a batch launch share a template's
 * waves).  mode 0 / 1 forces the first / the second (the second wherever a frame's top level fits a workgroup: 32768 positions), -1 leaves
 * it to the launcher's rule (the process-wide default is LM_COARSE_BATCH).  lm_detector_get_coarse_batch: 1 when the
 * last such coarse pass ran k_coarse_bits_batch.  Results never depend on it. */
int lm_detector_set_coarse_batch(lm_detector *d, int mode);
int lm_detector_get_coarse_batch(const lm_detector *d);
/* Tests: the number of coarse candidates per frame the buffers are first laid out for (default 262144, at least 1024; before the first
 * match only).  A frame that produces more is reported by lm_detector_collect as LM_ERR_OVERFLOW and the capacity grows, as ever. */
int lm_detector_set_candidate_capacity(lm_detector *d, int candidates);
/* Tests: the coarse candidates of collected frame `frame_no` (counted like lm_detector_frames_submitted) as the coarse kernel left them in
 * the frame's result slot, four words per slot: x, y, the bits of the float score, the work-list index.  Returns the number the frame
 * PRODUCED (its counter; more than the capacity after an overflow) and copies min(produced, candidate capacity, capacity) records.
 * LM_ERR_INVALID once the slot serves a later frame or the buffers have grown. */
int64_t lm_detector_read_candidates(lm_detector *d, uint64_t frame_no, int32_t *dst, int64_t capacity);
int lm_detector_last_timings(const lm_detector *d, lm_timings *t);

/* Test/diagnostic access to the device-resident intermediates of the last front end run (parity
 * tests compare them byte-for-byte with the oracle).  kind: 0 quantised colour, 1 quantised
 * normals (W_l*H_l bytes each), 2 linear memories colour, 3 linear memories normals
 * (8*W_l*H_l bytes each; built on demand when the last match ran on bit planes only), 4 the strip
 * records of a level below the top (colour block, normal block: [label][phase][strip][row] 8-byte
 * records of 32 cells x {response is 1, response is 4}), 5 the pair stream of the top level ({is-1
 * dword, is-4 dword} per 32 bytes of the flat linear memories, both modality blocks with their zero
 * tails) — 4 and 5 only after a match that used them (k_local_bits / k_coarse_bits; a stream the front
 * end wrote directly is cleared by the match unless lm_detector_set_direct_bits(d, 2) was set), 6 / 7
 * the second set of the wide paths in the layout and size of 4 / 5 (after a match on k_local_wide /
 * k_coarse_wide: with v the response of a cell, kinds 4 / 5 then hold {v & 1, v == 4} and kinds 6 / 7
 * {(v >> 1) & 1, nothing}; LM_ERR_INVALID while no such match has allocated them), 8 the quantised
 * normals of level 0 BEFORE the 5x5 median (W_0*H_0 bytes, 0 or one-hot; level 0 only): what the last
 * synchronous front end — a training view, a lone match, the first frame of a batch — left there.
 * Copies min(capacity, size) bytes, returns the full size. */
int64_t lm_detector_read_stage(lm_detector *d, int level, int kind, uint8_t *dst, int64_t capacity);

/* Canonical merge of match lists gathered from several ranks (LL.cpp:1771-1776 semantics, A12).
 * In-place on `m` (n entries); returns the new count. */
size_t lm_merge_matches(lm_match *m, size_t n);

/* Caller-side box NMS of the reference driver (linemod_and_levelup_test.py:34-61), numpy `nms`
 * semantics (+1 pixel convention, IoU > thresh suppresses, score-descending, stable for ties by
 * input order as numpy argsort()[::-1] is NOT guaranteed — ties broken by higher index first).
 * boxes: [n][4] float64 x1,y1,x2,y2; scores [n] float64.  keep: [n] int32 out; returns #kept. */
int lm_nms_boxes(const double *boxes, const double *scores, int n, double thresh, int32_t *keep);
/* Translation NMS over refined poses, numpy `nms_norms` of linemod_ros/detect.py:41-51 (used at :128 with thresh 40.0 on
 * poseRefine translations, score = -residual): score-descending, a later pose survives iff ||t_i - t_j|| > thresh.
 * ts: [n][3] float64.  keep: [n] int32 out; returns #kept. */
int lm_nms_norms(const double *ts, const double *scores, int n, double thresh, int32_t *keep);
/* cv::dnn::NMSBoxes on integer rectangles as linemodLevelup/test.cpp:132-144 calls it (40x40 boxes, score_threshold 0,
 * nms_threshold 0.4): the published algorithm of OpenCV 3.4 dnn (NMSFast_) — OpenCV is un-vendored and unpinned, so
 * parity is with that algorithm, not with a binary.  rects: [n][4] int32 x, y, width, height; eta = 1, top_k = 0 are
 * OpenCV's defaults.  keep: [n] int32 out; returns #kept. */
int lm_nms_boxes_cv(const int32_t *rects, const float *scores, int n, float score_threshold, float nms_threshold, float eta,
                    int top_k, int32_t *keep);

void lm_free(void *p);

/* ---- poseRefine (pybind11.cpp:9-14, LL.cpp:27-170) ------------------------------------------
 * scene/model depth: uint16 [height][width] mm; K matrices float32 row-major 3x3; R float32 3x3,
 * t float32 3 (mm).  Outputs: R_out float64 3x3, t_out float64 3 (mm), residual (= ICP fitness,
 * or -1 when the detection window leaves the frame, LL.cpp:52-55).
 * flags: bit0 = LM_ICP_SCENE_FROM_SCENE: register against the SCENE cloud (evident intent) instead
 * of reproducing LL.cpp:109, which down-samples the model cloud twice.
 * bit1 = LM_ICP_POINT_TO_POINT: TransformationEstimationPointToPoint (the reference built without USE_OPEN3D_P2PL,
 * LL.cpp:132-134) instead of TransformationEstimationPointToPlane: the same correspondences, fitness and inlier RMSE, the
 * update [R | t] of Eigen::umeyama without scaling (identity when there are fewer than 3 correspondences or it is not
 * finite).  Such hypotheses run the sliced launches (stage 3).
 * Public flag bits live in flags & 0xFF; 0x100 is internal. */
#define LM_ICP_SCENE_FROM_SCENE 1
#define LM_ICP_POINT_TO_POINT 2
typedef struct lm_pose_result {
    double R[9];
    double t[3];
    float residual;      /* fitness; -1 = rejected */
    float inlier_rmse;
    int32_t iterations;
    int32_t n_source;    /* points after voxel down-sampling */
    int32_t n_target;
    int32_t stage;       /* the ICP stage that finished it: 1 first team launch (relaunch included), 2 large team builds,
                            3 sliced launches (LM_ICP_SLICED=1: all); 0 not registered */
} lm_pose_result;

int lm_pose_refine(int device, const uint16_t *scene_depth, const uint16_t *model_depth, int width, int height,
                   const float *scene_K, const float *model_K, const float *model_R, const float *model_t,
                   int detect_x, int detect_y, int flags, lm_pose_result *result);

/* Batched form (top-K hypotheses of one frame, BASELINE config 3): `count` model depth images /
 * poses against one scene depth; cloud preparation, normals and all ICP iterations on the device,
 * one workgroup per hypothesis in the iteration kernel.  device_ms: HIP-event time of the device pipeline. */
int lm_pose_refine_batch(int device, const uint16_t *scene_depth, int width, int height, const float *scene_K,
                         int count, const uint16_t *const *model_depths, const float *model_Ks /*[count][9]*/,
                         const float *model_Rs /*[count][9]*/, const float *model_ts /*[count][3]*/,
                         const int32_t *detect_xy /*[count][2]*/, int flags, lm_pose_result *results,
                         float *device_ms /* may be NULL: HIP-event time of the ICP launches */);

/* ---- resident ICP context (batched poseRefine without per-call allocation) ------
 * The same computation as lm_pose_refine_batch (which is set_scene + set_models + run on a shared
 * per-device context), split so that depth images stay resident in HBM across calls: a frame's scene
 * depth is uploaded once, model depth renderings live in numbered slots and any number of
 * hypotheses may refer to a slot.  Everything of poseRefine::process after the argument checks
 * (LL.cpp:43-148) runs on the device in one stream without host round trips. */
typedef struct lm_icp lm_icp;
int lm_icp_create(int device, lm_icp **out);
void lm_icp_destroy(lm_icp *c);
/* open3d ICPConvergenceCriteria of a context (lm_icp_options_init: the defaults, 30 / 1e-6 / 1e-6).  max_iteration >= 0;
 * 0 is EvaluateRegistration (LL.cpp:111-115): no update, transformation_ = init_guess, fitness and inlier RMSE of that
 * guess, iterations 0, the pose returned is init_guess * init_base.  relative_fitness, relative_rmse: > 0 and finite.
 * Anything else: LM_ERR_INVALID, the context keeps what it had.  options == NULL restores the defaults.  Hypotheses of a
 * context with other than the default criteria run the sliced launches (stage 3).  lm_pose_refine and
 * lm_pose_refine_batch run a shared per-device context at the defaults. */
typedef struct lm_icp_options {
    int32_t max_iteration;
    int32_t reserved;
    double relative_fitness, relative_rmse;
} lm_icp_options;
void lm_icp_options_init(lm_icp_options *o);
int lm_icp_set_options(lm_icp *c, const lm_icp_options *options);
/* sceneDepth + sceneK of poseRefine::process (LL.cpp:27); defines the frame geometry (changing it drops the slots). */
int lm_icp_set_scene(lm_icp *c, const uint16_t *scene_depth, int width, int height, const float *scene_K);
/* modelDepth images (LL.cpp:27) into slots [first_slot, first_slot + count). */
int lm_icp_set_models(lm_icp *c, int first_slot, int count, const uint16_t *const *model_depths);
/* `count` hypotheses; model_slots == NULL means hypothesis i uses slot i.  Outputs as lm_pose_refine_batch. */
int lm_icp_run(lm_icp *c, int count, const int32_t *model_slots, const float *model_Ks /*[count][9]*/,
               const float *model_Rs /*[count][9]*/, const float *model_ts /*[count][3]*/,
               const int32_t *detect_xy /*[count][2]*/, int flags, lm_pose_result *results, float *device_ms);
/* Test/diagnostic read-back of the last run's device intermediates of one hypothesis.  kind: 0 source
 * cloud, 1 target cloud, 2 target normals (xyz triples, voxel order), 3 {init_guess t[3], T[16],
 * n_model, n_scene, grid_x, grid_y, cell, iterations, 8 phase cycle counts, team_note[4], n_source, n_target, 4 kNN cycle counts,
 * 4 voxel cycle counts, n_model, n_scene, 16 sort cycle counts, team_size, resume_it, build (the k_icp_team build that finished the
 * hypothesis, KP * 4 + SLAB * 2 + slabbed: 4 <1,false>, 6 / 7 <1,true>, 10 / 11 <2,true>, 22 / 23 <5,true>; 0 the sliced launches),
 * groups of the eight-workgroup voxel sort that finished the model cloud, the scene cloud, of the eight-workgroup grid sort (8: that path
 * prepared the cloud, less: the one-workgroup kernel did), target points handed to the whole-cloud kNN search, points its list had no room for (0: it holds every target)}, 4 the slices' partial sums of
 * the last two evaluations [2][64][32] (slots 29-31 of a slice: its shader cycles, search cycles, queued points), 5 the cumulants of the
 * k nearest neighbours per sorted target position [n_target][12], 6 the original (voxel-order) index of the target point at every sorted
 * position [n_target].  Copies min(capacity, size) doubles, returns the size. */
int64_t lm_icp_read_debug(lm_icp *c, int hypothesis, int kind, double *dst, int64_t capacity);

/* ---- per-frame pipeline --------------------------------------------------------
 * The loop of the reference driver, linemod_and_levelup_test.py:324-372, as one stream of device work:
 * Detector::match -> dets (x, y, x+width, y+height, similarity) of the matched templates (:331-339) ->
 * numpy nms(dets, 0.5) (:340, :34-61) -> for the first top_k kept matches poseRefine.process against
 * the depth rendering of the matched template view (:349-367).  The renderings (what the driver gets
 * from pysixd's renderer with aTemplateInfo[template_id]'s cam_K / cam_R_w2c / cam_t_w2c) are uploaded
 * once per template and stay in HBM; NMS, top-K, hypothesis set-up and ICP run on the device with no
 * host round trip.  Result = lm_detector_match + lm_nms_boxes + lm_pose_refine_batch on the same frame. */
typedef struct lm_pipeline lm_pipeline;
typedef struct lm_detection {
    lm_match match;          /* the kept match */
    int32_t width, height;   /* its NMS box: the template's size */
    int32_t status;          /* 0 refined; 1 detection window leaves the frame (residual -1, LL.cpp:52-55); 5 no view for this template */
    int32_t reserved;
    lm_pose_result pose;     /* refined pose (status 0) */
} lm_detection;
typedef struct lm_pipeline_timings {
    float match_ms, nms_ms, icp_ms, total_ms;   /* HIP events on the detector's stream */
    int64_t coarse_candidates, matches_pre_unique;
    int32_t icp_iterations;
    int32_t nms_records;     /* distinct (x, y, template, class) records the on-device NMS ran over; > 8192: they stayed in HBM, else in LDS */
} lm_pipeline_timings;
int lm_pipeline_create(lm_detector *det, int width, int height, lm_pipeline **out);
void lm_pipeline_destroy(lm_pipeline *p);
/* lm_icp_set_options on the pipeline's own ICP context. */
int lm_pipeline_set_icp_options(lm_pipeline *p, const lm_icp_options *options);
/* Views of templates [first_template, first_template + count) of a class: depth rendering (uint16 [height][width],
 * mm), cam_K, cam_R_w2c (float32 3x3 row-major), cam_t_w2c (float32 3, mm); box_wh: NULL, or [count][2] int32
 * aTemplateInfo 'width','height' (the NMS box of the driver, :335-338); NULL / negative = the template's own size. */
int lm_pipeline_set_views(lm_pipeline *p, const char *class_id, int first_template, int count,
                          const uint16_t *const *depth_ren, const float *Ks, const float *Rs, const float *ts,
                          const int32_t *box_wh);
/* Runs on the detector's resident frame (lm_detector_set_frame / select_frame).  out: top_k entries; *n_out kept. */
/* lm_icp_read_debug on the pipeline's own ICP context (the hypotheses of the last lm_pipeline_run). */
int64_t lm_pipeline_read_icp_debug(lm_pipeline *p, int hypothesis, int kind, double *dst, int64_t capacity);
int lm_pipeline_run(lm_pipeline *p, float threshold, const char *const *class_ids, int num_class_ids, const float *scene_K,
                    int top_k, double nms_iou, int flags, lm_detection *out, int *n_out, lm_pipeline_timings *tm);

/* ---- meshes and rendering --------------------------------------------------------
 * What the reference driver gets from pysixd: inout.load_ply (inout.py) and renderer.render
 * (renderer.py:306-420; linemod_and_levelup_test.py:206-215 for the training views, :352 for the depth_ren
 * poseRefine registers against).  The mesh lives in HBM; a batch of views is rasterised on the device
 * (depth at the native resolution; colour with per-fragment phong shading, light at the eye, at ssaa x the
 * resolution and box-averaged).  OpenCV camera convention: p_cam = R v + t, pixel (i, j) sampled at (i, j). */
typedef struct lm_mesh lm_mesh;
int lm_mesh_create(int device, const float *vertices /*[nv][3] mm*/, const float *normals /*[nv][3] or NULL*/,
                   const uint8_t *colors /*[nv][3] or NULL*/, int nv, const int32_t *faces /*[nf][3]*/, int nf, lm_mesh **out);
int lm_mesh_load_ply(int device, const char *path, lm_mesh **out);   /* ascii / binary_little_endian, triangles; texture_u/_v if present */
void lm_mesh_destroy(lm_mesh *m);
int lm_mesh_counts(const lm_mesh *m, int *nv, int *nf);
/* render(model, (width, height), K, R, t, clip_near, clip_far, ambient_weight, shading='phong') for `count` views.
 * Ks/Rs [count][9] float32 row-major, ts [count][3] (mm).  depth_out: uint16 [count][height][width] (mm, truncated
 * like depth.astype(np.uint16)) or NULL; rgb_out: uint8 [count][height][width][3] or NULL. */
int lm_mesh_render(lm_mesh *m, int count, int width, int height, const float *Ks, const float *Rs, const float *ts,
                   float clip_near, float clip_far, float ambient, int ssaa, uint16_t *depth_out, uint8_t *rgb_out);
/* The render_train loop of the driver (:170-252) without the round trip through host images: renders every view
 * (depth + colour), runs Detector::addTemplate on it (mask = depth > 0) and reports the template id per view (-1 where
 * no template could be extracted) plus the extent of the rendered depth (aTemplateInfo 'width','height', :229-236). */
int lm_detector_add_templates_rendered(lm_detector *d, lm_mesh *m, const char *class_id, int count, int width, int height,
                                       const float *Ks, const float *Rs, const float *ts, float clip_near, float clip_far,
                                       float ambient, int ssaa, int32_t *template_ids /*[count]*/, int32_t *box_wh /*[count][2] or NULL*/);
/* ---- the rest of renderer.render's signature (renderer.py:306: texture, surf_color, bg_color, shading) --------------
 * lm_mesh_render and lm_detector_add_templates_rendered above keep their behaviour byte for byte; the entry points below
 * take the options as a struct that starts with its own size (lm_render_options_init fills the defaults of
 * lm_mesh_render: phong, ambient 0.8, ssaa 4, clip 10 / 10000, black background; pysixd's own defaults are flat and
 * ambient 0.5).  The rules of every mode are stated in 6dpose_amd/csrc/render.hip ("shading options") and restated in
 * numpy by tests/render_shade_ref.py; like the existing modes they are this library's specification, because the
 * reference's result depends on the GL implementation. */
#define LM_SHADING_PHONG 0  /* interpolated vertex normals, one-sided: max(0, L.N) */
#define LM_SHADING_FLAT 1   /* face normal turned towards the camera (renderer.py:62), two-sided: |L.N| */
typedef struct lm_render_options {
    uint32_t size;          /* sizeof(lm_render_options); anything else -> LM_ERR_INVALID */
    int32_t shading;        /* LM_SHADING_* */
    int32_t use_texture;    /* colour = light * nearest texel at the interpolated uv (renderer.py:316-321); needs
                               lm_mesh_set_texcoords and lm_mesh_set_texture; vertex colours and surf_color are ignored */
    int32_t has_surf_color; /* surf_color replaces the vertex colours (renderer.py:324-333) */
    float surf_color[3];    /* r, g, b in [0, 1], quantised to 8 bits (rint(255 x)) */
    float bg_color[4];      /* r, g, b in [0, 1], quantised to 8 bits, given to uncovered supersamples before the box
                               average; a accepted and ignored */
    float ambient;          /* ambient_weight */
    int32_t ssaa;           /* 1..8 */
    float clip_near, clip_far;
} lm_render_options;
void lm_render_options_init(lm_render_options *o);
/* texture_u / texture_v per vertex (inout.py:249-293; lm_mesh_load_ply reads them when the file has them); count must
 * equal the number of vertices.  uv [count][2] float32; v = 1 is the top row of the texture image. */
int lm_mesh_set_texcoords(lm_mesh *m, const float *uv, int count);
/* The texture image, uint8 [height][width][3] as the caller sees it (row 0 = top; pysixd's np.flipud, renderer.py:319,
 * is part of the lookup rule).  Kept in HBM as 4-byte texels. */
int lm_mesh_set_texture(lm_mesh *m, const uint8_t *rgb, int width, int height);
int lm_mesh_texture_info(const lm_mesh *m, int *has_texcoords, int *width, int *height);   /* 0 x 0: no image */
/* lm_mesh_render with options.  LM_ERR_INVALID: unknown shading, a colour outside [0, 1], use_texture without texture
 * coordinates or image. */
int lm_mesh_render_ex(lm_mesh *m, int count, int width, int height, const float *Ks, const float *Rs, const float *ts,
                      const lm_render_options *options, uint16_t *depth_out, uint8_t *rgb_out);
/* lm_detector_add_templates_rendered with options: render_train for textured models (linemod_and_levelup_test.py:193-227
 * passes texture=model_texture) and other backgrounds. */
int lm_detector_add_templates_rendered_ex(lm_detector *d, lm_mesh *m, const char *class_id, int count, int width, int height,
                                          const float *Ks, const float *Rs, const float *ts, const lm_render_options *options,
                                          int32_t *template_ids /*[count]*/, int32_t *box_wh /*[count][2] or NULL*/);
/* Pose overlays (linemod_and_levelup_test.py:377-383, tools/vis_gt_poses.py:120-145): pose i = meshes[i] at (Rs[i], ts[i])
 * rendered at the frame's size with `options` (ssaa must be 1) and surface colour surf_colors[i] ([count][3] in [0, 1], or
 * NULL for the mesh's own colours), then composed into a copy of rgb on the device: one batch of renders per distinct
 * mesh and one compose kernel.  A pose shows at a pixel where its rendered depth is > 0 and, with scene_depth (uint16 mm,
 * or NULL), where scene_depth == 0 or depth < scene_depth (the driver's visible_mask, :379).  PAINTER: the last such
 * pose wins (the driver's paste order); NEAREST: the smallest rendered depth wins, the lower index on a tie
 * (vis_gt_poses' resolve_visib).  rgb_out uint8 [height][width][3]; index_out int8 [height][width], -1 where no pose
 * shows.  1 <= count <= 127. */
#define LM_OVERLAY_PAINTER 0
#define LM_OVERLAY_NEAREST 1
int lm_mesh_overlay(lm_mesh *const *meshes, int count, int width, int height, const uint8_t *rgb, const float *Ks,
                    const float *Rs, const float *ts, const float *surf_colors, const lm_render_options *options,
                    const uint16_t *scene_depth, int mode, uint8_t *rgb_out, int8_t *index_out);
/* Views of a pipeline rendered on the device: depth_ren of template first_template + i = the mesh at (Rs[i], ts[i]). */
int lm_pipeline_set_views_rendered(lm_pipeline *p, lm_mesh *m, const char *class_id, int first_template, int count,
                                   const float *Ks, const float *Rs, const float *ts, float clip_near, float clip_far,
                                   const int32_t *box_wh);

/* ---- pose errors (pysixd/pose_error.py, tools/eval_calc_errors.py:142-178, tools/calc_gt_stats.py:103-155) ----------
 * The batch E estimates x G ground truths of one object in one frame.  Poses: R [n][9] row-major f64, t [n][3] f64 (mm);
 * K [9] f64.  Renders use R, t and K cast to float32 and the rasteriser of lm_mesh_render (float32 eye depth read from
 * its z-buffer, not the truncated uint16 image); distance images, visibility and costs follow pysixd (DESIGN.md,
 * "Pose errors").  scene_depth: float32 [height][width] in mm (load_depth * depth_scale). */
#define LM_POSE_VSD 1   /* needs scene_depth, K, width, height; delta, tau, cost */
#define LM_POSE_COU 2   /* needs K, width, height */
#define LM_POSE_ADD 4
#define LM_POSE_ADI 8
#define LM_POSE_RE 16
#define LM_POSE_TE 32
#define LM_POSE_MSSD 64   /* lm_mesh_pose_errors_sym only */
#define LM_POSE_MSPD 128  /* lm_mesh_pose_errors_sym only; needs K */
#define LM_POSE_COST_STEP 0
#define LM_POSE_COST_TLINEAR 1
/* out: f64 [n_metrics][n_est][n_gt], the requested metrics in the order of their bits (VSD, COU, ADD, ADI, RE, TE).
 * VSD without scene_depth -> LM_ERR_INVALID.  n_est == 0 or n_gt == 0 writes nothing.  pysixd renders with
 * clip_near = 100, clip_far = 10000 for VSD and COU (pose_error.py:35-39). */
int lm_mesh_pose_errors(lm_mesh *m, int n_est, const double *R_est, const double *t_est, int n_gt, const double *R_gt,
                        const double *t_gt, const double *K, int width, int height, const float *scene_depth, int metrics,
                        double delta, double tau, int cost, double clip_near, double clip_far, double *out);
/* Symmetry-aware errors of the BOP toolkit (maximum symmetry-aware surface / projection distance), for the mesh's
 * vertices v (float32 on the device, widened to f64) and an explicit set of n_sym >= 1 symmetry transformations
 * (R_sym [n_sym][9] row-major, t_sym [n_sym][3] mm; the identity is an entry like any other):
 *   MSSD[e][g] = min_s max_v || (R_e v + t_e) - (R_g (R_s v + t_s) + t_g) ||                       (mm)
 *   MSPD[e][g] = min_s max_v || proj(R_e v + t_e) - proj(R_g (R_s v + t_s) + t_g) ||               (pixels)
 *   proj(p) = ((K p)[0] / (K p)[2], (K p)[1] / (K p)[2])
 * f64 throughout; max and min only, so two calls are bit-identical.  metrics: LM_POSE_MSSD | LM_POSE_MSPD; out: f64
 * [n_metrics][n_est][n_gt], MSSD then MSPD.  K may be NULL without MSPD.  A point with (K p)[2] <= 0 is the caller's
 * problem, as in numpy: the division is carried out as it stands.  LM_ERR_INVALID: n_sym < 1, MSPD without K, other bits. */
int lm_mesh_pose_errors_sym(lm_mesh *m, int n_est, const double *R_est, const double *t_est, int n_gt, const double *R_gt,
                            const double *t_gt, int n_sym, const double *R_sym, const double *t_sym, const double *K,
                            int metrics, double *out);
/* Symmetry transformations lm_mesh_pose_errors_sym stages in LDS at once; larger sets are swept in tiles of this size. */
int lm_pose_sym_tile(void);
/* calc_gt_stats.py:103-155 for each GT pose: counts [n_gt][3] = px_count_all, px_count_valid, px_count_visib;
 * visib_fract [n_gt]; bbox_obj, bbox_visib [n_gt][4] = x, y, w, h (misc.calc_2d_bbox; -1s when nothing is visible).
 * pysixd renders with its defaults clip_near = 100, clip_far = 2000 here (renderer.py:306). */
int lm_mesh_gt_stats(lm_mesh *m, int n_gt, const double *R_gt, const double *t_gt, const double *K, int width, int height,
                     const float *scene_depth, double delta, double clip_near, double clip_far, int64_t *counts,
                     double *visib_fract, int32_t *bbox_obj, int32_t *bbox_visib);
/* misc.calc_pts_diameter: the largest vertex-to-vertex distance (mm). */
int lm_mesh_diameter(lm_mesh *m, double *diameter);

/* ---- pose refinement by particle swarm over rendered depth (linemodLevelup/readme.md:41-46, the author's todo) ----------
 * Correspondence-free: each of `count` hypotheses (R0, t0) gets P particles x = (dt[3] mm, a[3]), a a Cayley rotation
 * vector, dR(a) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a); the particle's pose is R = dR(a) R0, t = t0 + dt.  Every
 * particle is rendered depth-only (the rasteriser of lm_mesh_render) into a w x h window of the frame whose origin is the
 * hypothesis' windows_xy, and scored against the scene depth there: over pixels with rendered depth r > 0 (n_r of them) the
 * sum of tau where the scene depth s is 0 and min(|r - s|, tau) elsewhere; cost = sum / n_r when n_r >= (n_0 + 1) / 2 and
 * n_r > 0, else +inf (n_0: the n_r of the given pose, so that a particle cannot win by leaving the view).  Window pixels
 * outside the frame read s = 0.  The swarm, its random numbers and every operation's order are stated in numpy by
 * tests/pso_ref.py, which is this refiner's specification; the device follows it bit for bit, so a call is repeatable and
 * depends on the seed alone.  A call is one enqueue on the context's stream with no host synchronisation before the copy
 * of the results.  LM_ERR_INVALID: the limits stated in amd_linemod_pso.h, 8 <= w, h <= 256, count x P <= 4096, a mesh on
 * another device, no scene set. */
typedef struct lm_pso lm_pso;
void lm_pso_options_init(lm_pso_options *options);
int lm_pso_create(int device, lm_pso **out);
void lm_pso_destroy(lm_pso *c);
/* The scene depth (uint16 [height][width], mm, 0 = no measurement) and its camera K (float64 row-major 3x3); stays in HBM. */
int lm_pso_set_scene(lm_pso *c, const uint16_t *scene_depth, int width, int height, const double *K);
/* Rs [count][9], ts [count][3] float64; windows_xy [count][2] int32 (may leave the frame); options NULL = the defaults. */
int lm_pso_run(lm_pso *c, lm_mesh *mesh, int count, const double *Rs, const double *ts, const int32_t *windows_xy /*[count][2]*/,
               int w, int h, const lm_pso_options *options, lm_pso_result *results, float *device_ms);
/* Test/diagnostic read-back of the last run's record of one hypothesis, generation 0 (the initial swarm) to `generations`.
 * kind: 0 the positions evaluated x [G + 1][P][6], 1 their costs [G + 1][P], 2 (sum, n_r) [G + 1][P][2], 3 (particle,
 * generation) of the global best after each generation [G + 1][2].  Integers are returned as doubles, doubles bit for bit.
 * Copies min(capacity, size) doubles, returns the size. */
int64_t lm_pso_read_debug(lm_pso *c, int hypothesis, int kind, double *dst, int64_t capacity);
/* ---- the same swarm scored against the scene's edges: for cameras without depth (chamfer cost) ---------------------------
 * The scene is an edge map (uint8 [height][width], a pixel is an edge where it is not 0) with a camera K of its own.
 * lm_pso_set_scene_edges uploads it and computes, once, D2 [height][width] uint16: the squared distance in pixels to the
 * nearest edge pixel, truncated at max_dist (1..255; 32 is a sound default): D2 = min(max_dist^2, (x - x')^2 + (y - y')^2),
 * max_dist^2 everywhere on a map without edges.  The edge scene and the depth scene of lm_pso_set_scene are independent:
 * a context may hold either or both, of different sizes, and neither call disturbs the other. */
int lm_pso_set_scene_edges(lm_pso *c, const uint8_t *edges, int width, int height, const double *K, int max_dist);
/* Test/diagnostic read-back of D2.  Copies min(capacity, width x height) values, returns width x height. */
int64_t lm_pso_read_edge_distance(lm_pso *c, uint16_t *dst, int64_t capacity);
/* lm_pso_run with the edge cost; arguments, options, limits and the record for lm_pso_read_debug as there.  A pixel of a
 * particle's rendered window is a contour pixel iff its depth r > 0 and one of its four neighbours n inside the window has
 * n == 0 or, with edge_step_mm > 0, n - r > edge_step_mm (the near side of a depth jump of the model, so a self-occlusion
 * edge counts once; 0 = the silhouette only).  Neighbours outside the window are ignored.  A contour pixel adds
 * min(D2, tau^2) at its place in the frame, tau^2 outside the frame; options->tau is read as pixels, 1 <= tau <= max_dist.
 * cost = sum / n_c (px^2) over the n_c contour pixels, under the same cover floor with contour counts: n_rendered and
 * n_initial of the results are contour pixel counts, and kind 2 of lm_pso_read_debug is (sum, n_c).  The rule is stated in
 * numpy by tests/pso_edges_ref.py and followed bit for bit.  LM_ERR_INVALID in addition: no edges set, tau > max_dist,
 * edge_step_mm outside 0..65535. */
int lm_pso_run_edges(lm_pso *c, lm_mesh *mesh, int count, const double *Rs, const double *ts, const int32_t *windows_xy /*[count][2]*/,
                     int w, int h, const lm_pso_options *options, int edge_step_mm, lm_pso_result *results, float *device_ms);
/* ---- the edge cost with orientations: directional chamfer matching (Liu et al., Fast Directional Chamfer Matching) -------
 * The scene is Q (uint8 [height][width]) with a camera K of its own: bit k (0..7) of a pixel set = an edge of orientation
 * bin k there, LINE-MOD's quantised colour gradients (what lm_detector_read_stage(level, 0) reads); several bits may be set,
 * 0 = no edge.  lm_pso_set_scene_orientations uploads it and computes, once, nine planes DD2 [9][height][width] uint16.  With
 * D2_j the truncated squared distance of lm_pso_set_scene_edges to the pixels with bit j, P = orient_penalty (0..4096 px^2
 * per bin^2; 16 — one bin off costs as much as 4 px — is a choice, not a measurement) and d(k, j) = min(|k - j|, 8 - |k - j|):
 * DD2[k] = min(max_dist^2, min over j of D2_j + P d(k, j)^2), k = 0..7, the squared distance in (x, y, sqrt(P) bin) to the
 * nearest oriented edge; DD2[8] = min over j of D2_j, what lm_pso_set_scene_edges computes for Q != 0.  The oriented scene
 * is independent of the depth scene and of the edge scene of the same context.  LM_ERR_INVALID: max_dist outside 1..255,
 * orient_penalty outside 0..4096. */
int lm_pso_set_scene_orientations(lm_pso *c, const uint8_t *Q, int width, int height, const double *K, int max_dist,
                                  int orient_penalty);
/* The same from the detector's last front end, on the device: the quantised colour map of pyramid `level` is copied device to
 * device once the detector's streams are idle, then transformed; no byte of it crosses PCIe.  The frame is that level's
 * (the aligned size >> level), K the camera of that level.  LM_ERR_INVALID in addition: frames in flight on the detector,
 * no front end has run on it, its modality set has no ColorGradient, it lives on another device than the context. */
int lm_pso_set_scene_from_detector(lm_pso *c, lm_detector *det, int level, const double *K, int max_dist, int orient_penalty);
/* Test/diagnostic read-back of one plane (0..8) of DD2.  Copies min(capacity, width x height) values, returns width x height. */
int64_t lm_pso_read_orient_distance(lm_pso *c, int plane, uint16_t *dst, int64_t capacity);
/* lm_pso_run_edges against the oriented scene.  The contour pixels are lm_pso_run_edges' own.  For a contour pixel of depth r,
 * o(n) = 1 for each of its 8 neighbours n that lies inside the window and has n == 0 or, with edge_step_mm > 0,
 * n - r > edge_step_mm, else 0; (gx, gy) are the 3 x 3 Sobel sums of o, y downwards, and the pixel's bin is
 * k = round(atan2(gy, gx) in degrees mod 360 * 16 / 360) & 7, the front end's own quantisation, from an exact table.  The pixel
 * adds min(DD2[k], tau^2) at its place in the frame, DD2[8] where gx == gy == 0, tau^2 outside the frame; everything else is
 * lm_pso_run_edges'.  The rule is stated in numpy by tests/pso_orient_ref.py and followed bit for bit; with orient_penalty 0
 * a call returns what lm_pso_run_edges returns on Q != 0.  LM_ERR_INVALID in addition: no orientations set, tau > max_dist. */
int lm_pso_run_oriented(lm_pso *c, lm_mesh *mesh, int count, const double *Rs, const double *ts, const int32_t *windows_xy /*[count][2]*/,
                        int w, int h, const lm_pso_options *options, int edge_step_mm, lm_pso_result *results, float *device_ms);

#ifdef __cplusplus
}
#endif
#endif /* AMD_LINEMOD_H */
