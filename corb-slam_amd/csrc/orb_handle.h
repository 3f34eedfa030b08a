// orb_handle.h -- the batched extractor's handle (corb_orb.cpp) and its part-batch scheduling, shared with the front-ends built on it
// (the stereo front-end in corb_orb.cpp, the RGB-D / monocular front-end in corb_cam.cpp).  Host code only.
#pragma once
#include "corb_internal.h"
#include <algorithm>
#include <mutex>
#include <vector>

#include "owned_hip.h"

struct CorbOrb {
    int device = 0;             // cfg.device
    CorbOrbConfig cfg;
    CorbOrbParams p;            // host copy
    CorbOrbParams* dp = nullptr;
    OwnedStream stream;
    // A run of many images is issued as `parts` part-batches, part 0 on `stream`, part i on side[i-1]; part i starts when part i-1 has
    // launched its FAST kernel (ev_stage), so the parts run half a pipeline apart and the VALU-bound kernels of one meet the
    // latency-bound kernels of the other.  The side streams are joined into `stream` lazily (corb_join), by the next call that touches the
    // results or the inputs -- back-to-back runs keep their phase offset.
    OwnedStream side[CORB_MAX_PARTS - 1];
    OwnedEvent ev_stage[CORB_MAX_PARTS], ev_done[CORB_MAX_PARTS - 1];
    int parts = 0;                                // 0: two parts (corb_run_parts); CORB_PARTS fixes another count
    int last_np = 0, max_np = 0;                  // parts of the previous split run; most parts (side streams in use) so far
    bool join_pending = false;
    int last_parts_images = 0;        // images of the last split run (its part boundaries follow from this and last_np)
    size_t octree_lds = 0;
    float scale[CORB_MAX_LEVELS], inv_scale[CORB_MAX_LEVELS], sigma2[CORB_MAX_LEVELS], inv_sigma2[CORB_MAX_LEVELS];
    int quota[CORB_MAX_LEVELS];
    int umax[16];
    int last_n_images = 0;
    DevList allocs;
    CorbProfiler prof;
    std::mutex stage_mu;        // guards the pinned staging area below
    PinnedMem h_status, h_count;                 // [max_images] ints
    // pinned staging of ONE image's input and outputs: the single-image operator (corb_orb_extract) and the fetch calls move their
    // data with true asynchronous DMA and one synchronisation instead of several pageable copies
    DevMem d_stage;                              // device staging of one contiguous input image (re-pitched by orb_ingest_kernel)
    DevMem d_stage_batch;                        // staging of a whole batch (corb_orb_upload_batch), allocated on first use: the bytes asked for and 256 more
    PinnedMem h_img, h_kp, h_desc, h_f32, h_misc;      // bytes, CorbKeyPoint, bytes, floats, 8 ints
    DevMem d_cand_tmp, d_cand_n;                 // CorbKeyPoint of the largest request; one int
};

// device allocation owned by the handle (freed by corb_orb_destroy)
template <class T> static int dalloc(CorbOrb* h, T** out, size_t n)
{
    const hipError_t e = h->allocs.add(reinterpret_cast<char**>(out), n * sizeof(T) + 256);
    if (e != hipSuccess) { corb_set_error("hipMalloc(%zu) failed: %s", n * sizeof(T) + 256, hipGetErrorString(e)); return CORB_ERR_HIP; }
    return CORB_OK;
}

// A run of >= CORB_SPLIT_MIN images is issued as part-batches on the handle's stream and its side streams, staggered by the stage events
// (see CorbOrb).  To the caller it is still one asynchronous operation on the handle: every entry point that reads results or rewrites
// inputs joins the side streams first.
#ifndef CORB_SPLIT_MIN
#define CORB_SPLIT_MIN 32
#endif
static inline void corb_join(CorbOrb* h)
{
    if (!h->join_pending) return;
    for (int i = 0; i < h->max_np - 1; i++) (void)hipStreamWaitEvent(h->stream, h->ev_done[i], 0);
    h->join_pending = false;
}
// side stream i, created on first use: HIP multiplexes streams onto a few hardware queues, and an idle extra stream per handle made two handles' streams
// share queues (the pipelined host-buffer mode of bench.py lost its transfer / compute overlap: 42.9 k -> 27.6 k fps)
static inline hipStream_t corb_side(CorbOrb* h, int i)
{
    if (!h->side[i]) {
        (void)h->side[i].create();
        (void)h->ev_done[i].create(hipEventDisableTiming);
    }
    return h->side[i];
}
// units [0, n) (images: ipu = 1, or stereo frames: ipu = 2 images per unit) as parts: launch(first_unit, n_units, stream, stage_event) enqueues one part.
// TWO parts at every size (round 4, tools/gpu_step_sweep.sh, profiles/r04_step_sweep.txt; stereo frames per run -> k stereo fps at 2 / 3 / 4 parts): 128 -> 97.1 / 97.3 /
// 87.8; 192 -> 98.5 / 98.8 / -; 256 -> 101.5 / - / 93.9; 384 -> 101.9; 512 -> 103.4 / 100.6 / 97.4; 768 -> 99.3; 1024 -> 97.2 / - / 98.0.  Larger parts have fewer launch tails
// to fill; more than two in flight only divide the wave slots further.  (Round 2 cut runs into parts of ~128 images: its pyramid kernel had 1 024-thread workgroups.)
template <class Launch>
static void corb_run_parts(CorbOrb* h, int n, int ipu, Launch launch)
{
    int np = h->parts > 0 ? h->parts : 2;
    np = std::min(np, n);
    // Back-to-back runs keep their stagger only when they cut the images the same way.  A run with other part boundaries (another n, another part count, or
    // unsplit) would touch images whose previous part is still in flight on a side stream: join first (free when nothing is pending).
    if (h->join_pending && (np <= 1 || h->last_np != np || h->last_parts_images != n * ipu)) corb_join(h);
    if (np <= 1) { launch(0, n, h->stream, (hipEvent_t) nullptr); return; }
    for (int i = 0; i < np; i++) {
        const int u0 = (int)((long long)n * i / np), u1 = (int)((long long)n * (i + 1) / np);
        hipStream_t st = i == 0 ? h->stream : corb_side(h, i - 1);
        if (i > 0) (void)hipStreamWaitEvent(st, h->ev_stage[i - 1], 0);          // inputs ready (part 0 follows the uploads) + half a pipeline behind part i-1
        // ... and the first part of THIS run stays behind the last part's FAST of the PREVIOUS run: without this second half of the handshake the lag of the
        // side stream is only bounded from below -- any disturbance (one profiled step was enough) let it drift to a full period, i.e. both parts in
        // lockstep, and back-to-back runs stayed in that mode: 81.5 k instead of 85 k fps
        else if (h->last_np > 1) (void)hipStreamWaitEvent(st, h->ev_stage[h->last_np - 1], 0);
        launch(u0, u1 - u0, st, h->ev_stage[i]);
        if (i > 0) (void)hipEventRecord(h->ev_done[i - 1], st);
    }
    h->last_np = np; h->last_parts_images = n * ipu; h->max_np = std::max(np, h->max_np);      // (side streams an earlier, larger run used keep their completed ev_done: joining them again is free)
    h->join_pending = true;
}
