/* The plain structures of depth-scaled matching (lm_detector_match_scaled of amd_linemod.h).
 * Included by amd_linemod.h; not meant to be included on its own. */
#ifndef AMD_LINEMOD_SCALED_H
#define AMD_LINEMOD_SCALED_H

#include <stdint.h>

#define LM_SCALED_MAX_SCALES 16

/* One record of lm_detector_match_scaled.  x, y, similarity, class_index and template_id are those of lm_match, in the UNSCALED convention:
 * with (w0, h0) the level-0 size of the template, the object's box has centre (x + w0 / 2, y + h0 / 2) and size scale * (w0, h0), scale =
 * scales_q10[scale_index] / 1024.  depth_mm is the probed scene depth the scale was chosen from. */
typedef struct lm_scaled_match {
    int32_t x;
    int32_t y;
    float similarity;
    int32_t class_index;
    int32_t template_id;
    int32_t scale_index;
    int32_t depth_mm;
} lm_scaled_match;

/* lm_scaled_options_init fills in a ladder of 9 (512 609 724 861 1024 1218 1448 1722 2048), bounds 0, 0 and probe 2. */
typedef struct lm_scaled_options {
    int32_t num_scales;                          /* 1..16 */
    int32_t scales_q10[LM_SCALED_MAX_SCALES];    /* strictly ascending, each in [512, 2048]; 1024 is scale 1 */
    int32_t min_scale_q10;                       /* 0: the first ladder entry; else in [1, 1048576] */
    int32_t max_scale_q10;                       /* 0: the last ladder entry; else in [min, 1048576] */
    int32_t probe;                               /* 0..4: the probe window is (2 probe + 1)^2 level-0 pixels */
} lm_scaled_options;

#endif /* AMD_LINEMOD_SCALED_H */
