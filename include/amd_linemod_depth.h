/* The plain structures of the depth-slab calls of amd_linemod.h (lm_detector_depth_modes, lm_detector_match_slabs).
 * Included by amd_linemod.h; not meant to be included on its own. */
#ifndef AMD_LINEMOD_DEPTH_H
#define AMD_LINEMOD_DEPTH_H

#include <stdint.h>

/* How the primary depths of a frame are found: a histogram of the depth image over [near_mm, far_mm) in bins of bin_mm, and a 1-D
 * non-maximum suppression over it.  lm_depth_mode_options_init fills in 25, 300, 4000, 2, 1000, 8. */
typedef struct lm_depth_mode_options {
    int32_t bin_mm;      /* >= 1 */
    int32_t near_mm;     /* >= 1: depth 0 is "no measurement" and counts nowhere */
    int32_t far_mm;      /* <= 65536; nbins = ceil((far_mm - near_mm) / bin_mm) in 1..4096 */
    int32_t window;      /* >= 0: bins on each side a mode has to dominate */
    int32_t min_pixels;  /* >= 1: pixels a bin needs to be a mode */
    int32_t max_modes;   /* 1..16: the modes with the most pixels are kept */
} lm_depth_mode_options;

/* One primary depth: its bin, the bin's centre near_mm + bin * bin_mm + bin_mm / 2, the pixels counted in the bin. */
typedef struct lm_depth_mode {
    int32_t bin;
    int32_t depth_mm;
    uint32_t pixels;
} lm_depth_mode;

/* One pass of lm_detector_match_slabs: the slab of a primary depth, or (depth_mm = -1, pixels = lo_mm = hi_mm = 0) the pass of the
 * classes without a depth range.  Its classes are slab_classes[first_class .. first_class + num_classes): positions in the requested
 * class list.  records: the records alive before any merge (lm_timings.matches_pre_unique of the pass); 0 for a slab no class wanted. */
typedef struct lm_slab {
    int32_t depth_mm;
    uint32_t pixels;
    int32_t lo_mm, hi_mm;
    int32_t first_class, num_classes;
    int64_t records;
} lm_slab;

#endif /* AMD_LINEMOD_DEPTH_H */
