// corb_cam.cpp -- C-ABI host side of the RGB-D / monocular front-end (see include/corb_accel.h): Frame::Frame(RGB-D) / Frame::Frame(monocular)
// (C/src/Frame.cc:119-228) with the input conversions of Tracking::GrabImageRGBD / GrabImageMonocular (C/src/Tracking.cc:206-264), built on the
// batched extractor (corb_orb.cpp).  No CPU compute fallback.
#include "cam_internal.h"
#include "orb_handle.h"
#include <cmath>
#include <cstring>
#include <map>

#include "host_util.h"

struct CorbRgbd {
    CorbOrb* orb = nullptr;
    CorbCamParams c;
    int max_frames = 0;
    float bounds[4] = {0, 0, 0, 0};          // mnMinX, mnMaxX, mnMinY, mnMaxY
    CorbRgbdFrameLayout lay;
    uint8_t* d_stage = nullptr;              // [max_frames][in_frame_bytes]: the captured chains read it, so it never moves
    uint8_t* d_result = nullptr;             // [max_frames][frame_bytes] (corb_rgbd_frames)
    std::map<int, hipGraphExec_t> frame_graph;
    OwnedEvent ev_t[4];
};

extern "C" int corb_rgbd_create(const CorbCameraConfig* cfg, CorbRgbd** out)
{
    if (!cfg || !out) { corb_set_error("corb_rgbd_create: null argument"); return CORB_ERR_ARG; }
    *out = nullptr;
    const bool rgbd = cfg->sensor == CORB_SENSOR_RGBD;
    if (cfg->max_frames < 1 || (cfg->sensor != CORB_SENSOR_RGBD && cfg->sensor != CORB_SENSOR_MONOCULAR) ||
        (cfg->channels != 1 && cfg->channels != 3 && cfg->channels != 4) || !(cfg->fx > 0) || !(cfg->fy > 0) ||
        (rgbd && (cfg->depth_format != CORB_DEPTH_U16 && cfg->depth_format != CORB_DEPTH_F32))) {
        corb_set_error("invalid CorbCameraConfig"); return CORB_ERR_ARG;
    }
    CorbOrbConfig oc = cfg->orb;
    oc.max_images = cfg->max_frames;
    CorbOrb* orb = nullptr;
    int rc = corb_orb_create(&oc, &orb);
    if (rc != CORB_OK) return rc;
    CorbRgbd* h = new CorbRgbd();
    h->orb = orb; h->max_frames = cfg->max_frames;
    CorbCamParams& c = h->c;
    memset(&c, 0, sizeof(c));
    c.w = oc.width; c.h = oc.height; c.channels = cfg->channels;
    c.blue_idx = cfg->rgb ? 2 : 0;                                   // CV_RGB2GRAY / CV_RGBA2GRAY: bidx 2; CV_BGR2GRAY / CV_BGRA2GRAY: bidx 0
    c.rgbd = rgbd ? 1 : 0;
    c.depth_f32 = cfg->depth_format == CORB_DEPTH_F32;
    // Tracking.cc:141-145 and :226-227, in the reference's float arithmetic
    float f = cfg->depth_map_factor;
    if (fabs(f) < 1e-5) f = 1;
    else f = 1.0f / f;
    c.depth_f = f;
    c.depth_convert = (fabs(f - 1.0f) > 1e-5) || !c.depth_f32;
    c.bf = cfg->bf;
    c.distorted = cfg->k1 != 0.0f;                                   // mDistCoef.at<float>(0) == 0.0 -> mvKeysUn = mvKeys (p1, p2, k3 are then ignored)
    // cvUndistortPoints: A = (double)K, k = (double)D (4 or 5 coefficients, the rest 0), RR = P * I as a double GEMM with P = K
    c.fx = (double)cfg->fx; c.fy = (double)cfg->fy; c.cx = (double)cfg->cx; c.cy = (double)cfg->cy;
    c.k[0] = cfg->k1; c.k[1] = cfg->k2; c.k[2] = cfg->p1; c.k[3] = cfg->p2; c.k[4] = cfg->k3 != 0.0f ? (double)cfg->k3 : 0.0;
    {
        const double P[9] = { c.fx, 0, c.cx, 0, c.fy, c.cy, 0, 0, 1 }, I[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                double s = 0;
                for (int k = 0; k < 3; k++) s += P[3 * i + k] * I[3 * k + j];
                c.RR[3 * i + j] = s;
            }
    }
    c.color_bytes = (size_t)c.w * c.h * c.channels;
    c.in_frame_bytes = c.color_bytes + (rgbd ? (size_t)c.w * c.h * (c.depth_f32 ? 4 : 2) : 0);
    c.cap = orb->p.out_cap;
    // Frame::ComputeImageBounds (Frame.cc:440-468): the four corners through the same undistortion
    if (c.distorted) {
        float u[4], v[4];
        const float cx4[4] = { 0.0f, (float)c.w, 0.0f, (float)c.w }, cy4[4] = { 0.0f, 0.0f, (float)c.h, (float)c.h };
        for (int i = 0; i < 4; i++) corb_undistort_point(c, cx4[i], cy4[i], &u[i], &v[i]);
        h->bounds[0] = std::min(u[0], u[2]); h->bounds[1] = std::max(u[1], u[3]);
        h->bounds[2] = std::min(v[0], v[1]); h->bounds[3] = std::max(v[2], v[3]);
    } else {
        h->bounds[0] = 0.0f; h->bounds[1] = (float)c.w; h->bounds[2] = 0.0f; h->bounds[3] = (float)c.h;
    }
    const size_t NF = (size_t)cfg->max_frames, cap = (size_t)c.cap;
    {
        // one frame's result block (corb_rgbd_frames): 64-byte header, then the five sections, each a multiple of 64 bytes
        auto a64 = [](size_t x) { return (int)((x + 63) & ~(size_t)63); };
        CorbRgbdFrameLayout& L = h->lay;
        L.capacity = (int)cap;
        L.input_bytes = (int)c.in_frame_bytes;
        int off = 64;
        L.off_keys = off; off += a64(cap * sizeof(CorbKeyPoint));
        L.off_keys_un = off; off += a64(cap * sizeof(CorbKeyPoint));
        L.off_desc = off; off += a64(cap * 32);
        L.off_u_right = off; off += a64(cap * sizeof(float));
        L.off_depth = off; off += a64(cap * sizeof(float));
        L.frame_bytes = off;
    }
    if (dalloc(orb, &h->d_stage, NF * c.in_frame_bytes) || dalloc(orb, &c.keys_un, NF * cap) || dalloc(orb, &c.u_right, NF * cap) || dalloc(orb, &c.depth, NF * cap) ||
        dalloc(orb, &h->d_result, NF * (size_t)h->lay.frame_bytes) ||
        hipMemset(h->d_result, 0, NF * (size_t)h->lay.frame_bytes) != hipSuccess) {
        corb_orb_destroy(orb); delete h; return CORB_ERR_HIP;
    }
    c.stage = h->d_stage;
    *out = h;
    return CORB_OK;
}

extern "C" void corb_rgbd_destroy(CorbRgbd* h)
{
    if (!h) return;
    CorbOrb* orb = h->orb;
    (void)corb_select_device(orb->device);
    if (orb->stream) (void)hipStreamSynchronize(orb->stream);
    for (auto& g : h->frame_graph) if (g.second) (void)hipGraphExecDestroy(g.second);
    delete h; corb_orb_destroy(orb);
}
extern "C" CorbOrb* corb_rgbd_orb(CorbRgbd* h) { return h ? h->orb : nullptr; }

extern "C" int corb_rgbd_frame_layout(CorbRgbd* h, CorbRgbdFrameLayout* out)
{
    if (!h || !out) return CORB_ERR_ARG;
    *out = h->lay;
    return CORB_OK;
}

extern "C" int corb_rgbd_image_bounds(CorbRgbd* h, float out[4])
{
    if (!h || !out) return CORB_ERR_ARG;
    for (int i = 0; i < 4; i++) out[i] = h->bounds[i];
    return CORB_OK;
}

extern "C" int corb_rgbd_upload_batch(CorbRgbd* h, int first_frame, int n_frames, const uint8_t* input)
{
    if (!h || !input || first_frame < 0 || n_frames < 1 || first_frame + n_frames > h->max_frames) { corb_set_error("corb_rgbd_upload_batch: bad argument"); return CORB_ERR_ARG; }
    CorbOrb* o = h->orb;
    HIPCHK(hipSetDevice(o->cfg.device));
    corb_join(o);
    HIPCHK(hipMemcpyAsync(h->d_stage + (size_t)first_frame * h->c.in_frame_bytes, input, (size_t)n_frames * h->c.in_frame_bytes, hipMemcpyHostToDevice, o->stream));
    corb_launch_cam_ingest(h->c, first_frame, n_frames, o->p, o->stream, o->prof.enabled ? &o->prof : nullptr);
    HIPCHK(hipGetLastError());
    return CORB_OK;
}

extern "C" int corb_rgbd_run(CorbRgbd* h, int n_frames)
{
    if (!h || n_frames < 1 || n_frames > h->max_frames) { corb_set_error("corb_rgbd_run: bad n_frames"); return CORB_ERR_ARG; }
    CorbOrb* o = h->orb;
    HIPCHK(hipSetDevice(o->cfg.device));
    CorbProfiler* prof = o->prof.enabled ? &o->prof : nullptr;
    auto launch = [&](int first, int n, hipStream_t st, hipEvent_t stage) {
        corb_launch_orb_pipeline(o->p, first, n, o->octree_lds, st, prof, stage);
        corb_launch_cam_finish(h->c, first, n, o->p, st, prof);
    };
    if (n_frames >= CORB_SPLIT_MIN && !o->prof.serial) corb_run_parts(o, n_frames, 1, launch);        // part-batches, see corb_orb_run
    else { corb_join(o); launch(0, n_frames, o->stream, nullptr); }
    HIPCHK(hipGetLastError());
    o->last_n_images = n_frames;
    return CORB_OK;
}

extern "C" int corb_rgbd_sync(CorbRgbd* h) { return h ? corb_orb_sync(h->orb) : CORB_ERR_ARG; }

extern "C" int corb_rgbd_fetch_batch(CorbRgbd* h, int first_frame, int n_frames, CorbKeyPoint* keys, CorbKeyPoint* keys_un, uint8_t* desc, float* u_right, float* depth,
                                     int32_t* counts)
{
    if (!h || !counts || first_frame < 0 || n_frames < 1 || first_frame + n_frames > h->max_frames) { corb_set_error("corb_rgbd_fetch_batch: bad argument"); return CORB_ERR_ARG; }
    CorbOrb* o = h->orb;
    HIPCHK(hipSetDevice(o->cfg.device));
    corb_join(o);
    const size_t cap = (size_t)o->p.out_cap, e0 = (size_t)first_frame * cap, ne = (size_t)n_frames * cap;
    hipStream_t st = o->stream;
    HIPCHK(hipMemcpyAsync(counts, o->p.out_count + first_frame, (size_t)n_frames * sizeof(int), hipMemcpyDeviceToHost, st));
    if (keys) HIPCHK(hipMemcpyAsync(keys, o->p.out_kp + e0, ne * sizeof(CorbKeyPoint), hipMemcpyDeviceToHost, st));
    if (keys_un) HIPCHK(hipMemcpyAsync(keys_un, h->c.keys_un + e0, ne * sizeof(CorbKeyPoint), hipMemcpyDeviceToHost, st));
    if (desc) HIPCHK(hipMemcpyAsync(desc, o->p.out_desc + e0 * 32, ne * 32, hipMemcpyDeviceToHost, st));
    if (u_right) HIPCHK(hipMemcpyAsync(u_right, h->c.u_right + e0, ne * sizeof(float), hipMemcpyDeviceToHost, st));
    if (depth) HIPCHK(hipMemcpyAsync(depth, h->c.depth + e0, ne * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return CORB_OK;
}

// Frame::Frame(RGB-D / monocular) as the reference's client calls it, per frame, in one call (see include/corb_accel.h).  The chain -- colour ingest, the ORB
// kernels on the n images unsplit, the finish and pack kernels -- depends on nothing but n and is captured once per n on the handle's one stream (no fork:
// the graph has no parallel branches), then replayed as ONE hipGraph launch between the two transfers.
extern "C" int corb_rgbd_frames(CorbRgbd* h, int n_frames, const uint8_t* input, void* result, CorbStereoFrameTiming* timing)
{
    if (!h || n_frames < 1 || n_frames > h->max_frames || !input || !result) { corb_set_error("corb_rgbd_frames: bad argument"); return CORB_ERR_ARG; }
    CorbOrb* o = h->orb;
    HIPCHK(hipSetDevice(o->cfg.device));
    corb_join(o);
    hipStream_t st = o->stream;
    if (timing && !h->ev_t[0]) for (auto& e : h->ev_t) HIPCHK(e.create(hipEventDefault));
    CorbProfiler* prof = o->prof.enabled ? &o->prof : nullptr;
    auto chain = [&](CorbProfiler* pr) {
        corb_launch_cam_ingest(h->c, 0, n_frames, o->p, st, pr);
        corb_launch_orb_pipeline(o->p, 0, n_frames, o->octree_lds, st, pr);
        corb_launch_cam_finish(h->c, 0, n_frames, o->p, st, pr);
        corb_launch_cam_pack(h->c, 0, n_frames, o->p, h->d_result, h->lay, st, pr);
    };
    if (timing) HIPCHK(hipEventRecord(h->ev_t[0], st));
    HIPCHK(hipMemcpyAsync(h->d_stage, input, (size_t)n_frames * h->c.in_frame_bytes, hipMemcpyHostToDevice, st));
    if (timing) HIPCHK(hipEventRecord(h->ev_t[1], st));
    if (prof) chain(prof);
    else {
        hipGraphExec_t& ge = h->frame_graph[n_frames];
        if (!ge) {
            hipGraph_t graph = nullptr;
            HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            chain(nullptr);
            HIPCHK(hipStreamEndCapture(st, &graph));
            const hipError_t e = hipGraphInstantiate(&ge, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (e != hipSuccess) { ge = nullptr; corb_set_error("corb_rgbd_frames: hipGraphInstantiate: %s", hipGetErrorString(e)); return CORB_ERR_HIP; }
        }
        HIPCHK(hipGraphLaunch(ge, st));
    }
    HIPCHK(hipGetLastError());
    if (timing) HIPCHK(hipEventRecord(h->ev_t[2], st));
    HIPCHK(hipMemcpyAsync(result, h->d_result, (size_t)n_frames * h->lay.frame_bytes, hipMemcpyDeviceToHost, st));
    if (timing) HIPCHK(hipEventRecord(h->ev_t[3], st));
    HIPCHK(hipStreamSynchronize(st));
    o->last_n_images = n_frames;
    if (timing) {
        (void)hipEventElapsedTime(&timing->ms_upload, h->ev_t[0], h->ev_t[1]);
        (void)hipEventElapsedTime(&timing->ms_kernels, h->ev_t[1], h->ev_t[2]);
        (void)hipEventElapsedTime(&timing->ms_download, h->ev_t[2], h->ev_t[3]);
    }
    for (int f = 0; f < n_frames; f++) {
        const int32_t* hd = reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(result) + (size_t)f * h->lay.frame_bytes);
        if (hd[1] != 0) { corb_set_error("frame %d: internal buffer overflow (status %d)", f, hd[1]); return CORB_ERR_OVERFLOW; }
    }
    return CORB_OK;
}

// device views of frame `frame`'s results for the keyframe store: mvKeysUn (what every device consumer reads), descriptors, mvuRight, mvDepth
int corb_rgbd_device_frame(CorbRgbd* h, int frame, CorbStereoDeviceFrame* out)
{
    if (!h || !out || frame < 0 || frame >= h->max_frames) return CORB_ERR_ARG;
    CorbOrb* o = h->orb; const size_t cap = (size_t)o->p.out_cap, e0 = (size_t)frame * cap;
    if (hipSetDevice(o->cfg.device) != hipSuccess) return CORB_ERR_HIP;
    corb_join(o);                                           // the consumer enqueues on o->stream
    out->kp = h->c.keys_un + e0; out->desc = o->p.out_desc + e0 * 32;
    out->u_right = h->c.u_right + e0; out->depth = h->c.depth + e0;
    out->count = o->p.out_count + frame; out->cap = (int)cap; out->stream = o->stream; out->device = o->cfg.device;
    return CORB_OK;
}
