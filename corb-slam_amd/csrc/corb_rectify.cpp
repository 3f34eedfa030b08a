// corb_rectify.cpp -- C-ABI host side of the stereo rectifier (include/corb_stereo_rectify.h): the maps of cv::initUndistortRectifyMap built once on the host
// (rectify_math.h), their fixed-point form on the device, and cv::remap of every raw pair as the first kernel of the stereo front-end's chain (corb_orb.cpp).
#include "host_util.h"
#include "orb_handle.h"
#include "rectify_internal.h"
#include "rectify_math.h"
#include "../../include/corb_stereo_rectify.h"
#include <cstring>
#include <map>
#include <vector>

struct CorbRect {
    int device = 0;
    CorbStereo* stereo = nullptr;      // borrowed
    CorbOrb* orb = nullptr;            // the stereo handle's extractor: its stream, its image slots
    int w = 0, h = 0, groups = 0, raw_w = 0, raw_h = 0, max_frames = 0;
    std::vector<float> map_x[2], map_y[2];                   // M1 / M2 per eye as built or set
    DevMem d_xy[2], d_frac[2];                               // rectify_internal.h: CorbRectParams
    DevMem d_raw;                                            // 2 * max_frames raw images; allocated at create, never replaced: the captured chains keep its address
    CorbRectParams P;
    std::map<int, hipGraphExec_t> graphs;                    // corb_rect_frames: the captured chain per frame count
};

// the float maps of one eye -> the kernel's two planes (host); false with a message at the first entry the conversion refuses
static bool rect_convert(const CorbRect* h, const float* mx, const float* my, std::vector<short2>& xy, std::vector<uint16_t>& frac, const char* who, int eye)
{
    const size_t row = (size_t)4 * h->groups;
    xy.assign(row * h->h, make_short2(-2, -2)); frac.assign(row * h->h, 0);               // (the entries past the width: outside, never stored)
    for (int i = 0; i < h->h; i++)
        for (int j = 0; j < h->w; j++) {
            RectFixed f;
            const float x = mx[(size_t)i * h->w + j], y = my[(size_t)i * h->w + j];
            if (!rect_fix(x, y, &f)) {
                corb_set_error("%s: map entry (%d, %d) of eye %d is (%g, %g): not finite, or 2^26 or more in magnitude", who, j, i, eye, (double)x, (double)y);
                return false;
            }
            xy[i * row + j] = make_short2(f.ix, f.iy); frac[i * row + j] = f.frac;
        }
    return true;
}

static int rect_install(CorbRect* h, int eye, const float* mx, const float* my, const std::vector<short2>& xy, const std::vector<uint16_t>& frac)
{
    hipStream_t st = h->orb->stream;
    HIPCHK(hipStreamSynchronize(st));                         // a chain in flight may still read the maps
    HIPCHK(hipMemcpy(h->d_xy[eye].as<void>(), xy.data(), xy.size() * sizeof(short2), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_frac[eye].as<void>(), frac.data(), frac.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    const size_t n = (size_t)h->w * h->h;
    h->map_x[eye].assign(mx, mx + n); h->map_y[eye].assign(my, my + n);
    return CORB_OK;
}

static bool all_zero(const double* v, int n) { for (int i = 0; i < n; i++) if (v[i] != 0.0) return false; return true; }

extern "C" int corb_rect_create(const CorbRectifyConfig* cfg, CorbStereo* stereo, CorbRect** out)
{
    if (!cfg || !stereo || !out) { corb_set_error("corb_rect_create: null argument"); return CORB_ERR_ARG; }
    *out = nullptr;
    CorbOrb* orb = corb_stereo_orb(stereo);
    const int w = orb->cfg.width, hgt = orb->cfg.height;
    // stereo_euroc.cc:88-93: "Calibration parameters to rectify stereo are missing!"
    if (cfg->raw_width < 1 || cfg->raw_height < 1 || w < 1 || hgt < 1) { corb_set_error("corb_rect_create: a zero image size"); return CORB_ERR_ARG; }
    if (cfg->raw_width > 32767 || cfg->raw_height > 32767 || w > 32767 || hgt > 32767) { corb_set_error("corb_rect_create: an image dimension above 32767"); return CORB_ERR_ARG; }
    const CorbRectifyEye* eyes[2] = {&cfg->left, &cfg->right};
    for (int e = 0; e < 2; e++)
        if (all_zero(eyes[e]->K, 9) || all_zero(eyes[e]->R, 9) || all_zero(eyes[e]->P, 12)) {
            corb_set_error("corb_rect_create: calibration parameters to rectify stereo are missing (eye %d: K, R or P is all zero)", e); return CORB_ERR_ARG;
        }
    std::vector<float> mx[2], my[2];
    std::vector<short2> xy[2]; std::vector<uint16_t> frac[2];
    CorbRect* h = new CorbRect();
    h->device = orb->cfg.device; h->stereo = stereo; h->orb = orb;
    h->w = w; h->h = hgt; h->groups = (w + 3) / 4; h->raw_w = cfg->raw_width; h->raw_h = cfg->raw_height; h->max_frames = orb->cfg.max_images / 2;
    for (int e = 0; e < 2; e++) {
        mx[e].resize((size_t)w * hgt); my[e].resize((size_t)w * hgt);
        if (!rect_build_maps(eyes[e]->K, eyes[e]->D, eyes[e]->R, eyes[e]->P, w, hgt, mx[e].data(), my[e].data())) {
            corb_set_error("corb_rect_create: eye %d: P3x3 * R has no inverse (its determinant is zero or not finite)", e); delete h; return CORB_ERR_ARG;
        }
        if (!rect_convert(h, mx[e].data(), my[e].data(), xy[e], frac[e], "corb_rect_create", e)) { delete h; return CORB_ERR_ARG; }
    }
    // every refusal is behind us: only now the device is touched
    if (hipSetDevice(h->device) != hipSuccess) { corb_set_error("corb_rect_create: hipSetDevice failed"); delete h; return CORB_ERR_HIP; }
    const size_t raw_bytes = (size_t)h->raw_w * h->raw_h * 2 * h->max_frames;
    bool ok = h->d_raw.room(raw_bytes + 256) == hipSuccess;
    for (int e = 0; e < 2 && ok; e++)
        ok = h->d_xy[e].room(xy[e].size() * sizeof(short2)) == hipSuccess && h->d_frac[e].room(frac[e].size() * sizeof(uint16_t)) == hipSuccess &&
             rect_install(h, e, mx[e].data(), my[e].data(), xy[e], frac[e]) == CORB_OK;
    if (!ok) { corb_set_error("corb_rect_create: device initialisation failed: %s", hipGetErrorString(hipGetLastError())); delete h; return CORB_ERR_HIP; }
    CorbRectParams& P = h->P;
    for (int e = 0; e < 2; e++) { P.xy[e] = h->d_xy[e].as<short2>(); P.frac[e] = h->d_frac[e].as<uint16_t>(); }
    P.w = w; P.h = hgt; P.groups = h->groups; P.raw_w = h->raw_w; P.raw_h = h->raw_h;
    *out = h;
    return CORB_OK;
}

extern "C" void corb_rect_destroy(CorbRect* h)
{
    if (!h) return;
    (void)corb_select_device(h->device);
    (void)hipStreamSynchronize(h->orb->stream);               // (the stream is the stereo handle's: that handle is destroyed after this one)
    for (auto& g : h->graphs) if (g.second) (void)hipGraphExecDestroy(g.second);
    delete h;
}

extern "C" int corb_rect_maps(CorbRect* h, int eye, float* map_x, float* map_y)
{
    if (!h || eye < 0 || eye > 1) { corb_set_error("corb_rect_maps: bad argument"); return CORB_ERR_ARG; }
    const size_t n = (size_t)h->w * h->h;
    if (map_x) memcpy(map_x, h->map_x[eye].data(), n * sizeof(float));
    if (map_y) memcpy(map_y, h->map_y[eye].data(), n * sizeof(float));
    return CORB_OK;
}

extern "C" int corb_rect_set_maps(CorbRect* h, int eye, const float* map_x, const float* map_y)
{
    if (!h || eye < 0 || eye > 1 || !map_x || !map_y) { corb_set_error("corb_rect_set_maps: bad argument"); return CORB_ERR_ARG; }
    std::vector<short2> xy; std::vector<uint16_t> frac;
    if (!rect_convert(h, map_x, map_y, xy, frac, "corb_rect_set_maps", eye)) return CORB_ERR_ARG;
    HIPCHK(hipSetDevice(h->device));
    corb_join(h->orb);
    return rect_install(h, eye, map_x, map_y, xy, frac);
}

static void rect_launch(CorbRect* h, int first_frame, int n_frames, hipStream_t st, CorbProfiler* prof)
{
    CorbOrb* o = h->orb; const CorbLevel& L0 = o->p.lv[0];
    const size_t frame_bytes = (size_t)2 * h->raw_w * h->raw_h;
    corb_launch_rect_remap(h->P, h->d_raw.as<uint8_t>() + first_frame * frame_bytes, 2 * n_frames,
                           o->p.pyr + (size_t)(2 * first_frame) * o->p.arena_per_image + L0.plane_off, L0.pitch, o->p.arena_per_image, st, prof);
}

extern "C" int corb_rect_upload_batch(CorbRect* h, int first_frame, int n_frames, const uint8_t* raw_left_right)
{
    if (!h || !raw_left_right || first_frame < 0 || n_frames < 1 || first_frame + n_frames > h->max_frames) { corb_set_error("corb_rect_upload_batch: bad argument"); return CORB_ERR_ARG; }
    CorbOrb* o = h->orb;
    HIPCHK(hipSetDevice(h->device));
    corb_join(o);
    const size_t frame_bytes = (size_t)2 * h->raw_w * h->raw_h;
    HIPCHK(hipMemcpyAsync(h->d_raw.as<uint8_t>() + first_frame * frame_bytes, raw_left_right, frame_bytes * n_frames, hipMemcpyHostToDevice, o->stream));
    rect_launch(h, first_frame, n_frames, o->stream, o->prof.enabled ? &o->prof : nullptr);
    HIPCHK(hipGetLastError());
    return CORB_OK;
}

extern "C" int corb_rect_frames(CorbRect* h, int n_frames, const uint8_t* raw_left_right, void* result, CorbStereoFrameTiming* timing)
{
    if (!h || n_frames < 1 || n_frames > h->max_frames || !raw_left_right || !result) { corb_set_error("corb_rect_frames: bad argument"); return CORB_ERR_ARG; }
    HIPCHK(hipSetDevice(h->device));
    corb_join(h->orb);
    CorbFrameInput in;
    in.who = "corb_rect_frames"; in.host = raw_left_right; in.bytes = (size_t)2 * h->raw_w * h->raw_h * n_frames; in.d_stage = h->d_raw.as<void>();
    in.planes = [](void* ctx, int n, hipStream_t st, CorbProfiler* prof) { rect_launch(static_cast<CorbRect*>(ctx), 0, n, st, prof); };
    in.ctx = h; in.graphs = &h->graphs;
    return corb_stereo_frames_chain(h->stereo, n_frames, in, result, timing);
}
