// Private view of the ICP context shared by pose_refine.cpp and pipeline.cpp (not part of the C ABI).
#pragma once
#include "../../include/amd_linemod.h"
#include "dev_buf.h"
#include "icp_kernels.h"
#include <vector>

using lm::IcpBuffers;
using lm::IcpIn;
using lm::IcpState;

struct lm_icp {
    int device = 0;
    DevStream s;                   // first: every event and buffer below dies before it (dev_buf.h)
    DevEvent e0, e1;
    int W = 0, H = 0;
    bool have_scene = false;
    float sK[9] = {0};
    int slots = 0;                 // resident model depth images
    int max_count = 0;             // hypotheses the arenas hold
    int last_count = 0, last_flags = 0;
    DevBuf<uint16_t> d_scene;      // [H][W]
    DevBuf<uint16_t> d_models;     // [slots][H][W]
    DevBuf<int> d_model_bbox;      // [slots][8] bounding box of a resident model depth image (x0, y0, x1, y1, state: 1 = known, -, -, -): worked out at upload (k_icp_model_boxes)
    std::vector<uint8_t> slot_boxed;   // host view of the state words: 1 = the slot's box was worked out at upload
    // What max_count hypotheses need, allocated together (lm_icp_ensure_arenas) and dropped together (`ar = {}`): the arenas under the
    // names and with the layouts of IcpBuffers, the hypothesis tables and their pinned twins.
    struct Arenas {
        DevBuf<double> model_pts, scene_pts, src, tgt, tgt_sorted, cov, normals, work, nn_lb, strip_sum, strip_mm, partial;
        DevBuf<int> tgt_orig, cell_start, prev_nn, strip_cnt;
        DevBuf<lm::TgtRec> tgt_rec;
        DevBuf<unsigned short> cell_start16;
        DevBuf<unsigned long long> strip_pub, keys, xchg;
        DevBuf<unsigned int> sort_look;
        DevBuf<IcpIn> in;
        DevBuf<IcpState> st;
        PinBuf<IcpIn> h_in;
        PinBuf<IcpState> h_st;     // the states uploaded before / read after a run
        PinBuf<IcpState> h_st2;    // read-back of lm_icp_run (h_st keeps the initial states for a repeated run)
    } ar;
    PinBuf<uint8_t> pinned;        // staging for images
    int cus = 0;                   // compute units of the device: the grid of k_icp_team
    bool sliced_only = false;      // LM_ICP_SLICED=1: RegistrationICP as one launch per evaluation (k_icp_eval, rounds 1-5), no k_icp_team
    std::vector<int> stage;        // per hypothesis of the last run: the lm::IcpStage that finished it
    lm_icp_options opt = {30, 0, 1e-6, 1e-6};   // ICPConvergenceCriteria (lm_icp_set_options)
    bool run_p2p = false;          // the run in flight: LM_ICP_POINT_TO_POINT
    int next_it = 0;               // the run in flight: first evaluation the sliced launches have not been enqueued for
    IcpBuffers buffers() const;    // what the kernels take, from the buffers as they are now; the caller sets scene, sK and count (pose_refine.cpp)
};


// pose_refine.cpp
// The ICP ladder of one run of B.count hypotheses on stream s, in two halves around the caller's synchronisation of s:
//   enqueue: the preparation of the clouds and the first stage (k_icp_team; the sliced launches under LM_ICP_SLICED=1, for
//            LM_ICP_POINT_TO_POINT in flags and for criteria other than the defaults), e1, then the read-back of the states into the
//            pinned h_st;
//   finish:  for what the first stage left unfinished the large team builds, then the sliced launches (64 evaluations at a time), each
//            followed by e1, the read-back and a synchronisation; a hypothesis still unfinished after those is an error.  Fills c->stage.
int lm_icp_enqueue(lm_icp* c, const lm::IcpBuffers& B, int flags, lm::IcpState* h_st, hipStream_t s);
int lm_icp_finish(lm_icp* c, const lm::IcpBuffers& B, lm::IcpState* h_st, hipStream_t s);
int lm_icp_set_geometry(lm_icp* c, int W, int H);      // (re)allocates for a frame size; drops the slots when it changes
int lm_icp_ensure_arenas(lm_icp* c, int count);        // arenas for `count` hypotheses
int lm_icp_ensure_slots(lm_icp* c, int slots);         // resident model depth images
// [R|t] of LL.cpp:34-41 and LL.cpp:146-154 from the device state of one hypothesis
void lm_icp_compose_result(const lm::IcpState& st, const float* model_R, const float* model_t, lm_pose_result* o);
