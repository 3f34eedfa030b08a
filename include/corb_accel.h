/* corb_accel.h -- C-ABI of the MI355X-native CORB-SLAM hot path (libcorb_accel.so).
 *
 * Plain C: opaque handles, POD structs, pointers + sizes, int status codes.  No exceptions.  An
 * extractor / stereo handle owns its device memory and its HIP streams (a run is issued as two
 * overlapping half-batches); the handle-less calls (matchers, optimisers, map maintenance) draw
 * device memory and stream from a per-device workspace with a short-call lane and a
 * long-optimisation lane.  Every function may be called from any host thread; calls on different
 * handles / lanes run concurrently (the reference calls the left/right extractors from two
 * std::threads, corbslam_client/src/Frame.cc:78-81, and its matchers / optimisers from the
 * Tracking, LocalMapping and LoopClosing threads).
 *
 * Citations are relative to the reference tree (lifunudt/CORB-SLAM):
 *   C/ = corbslam_client/   S/ = corbslam_server/   G/ = corbslam_client/Thirdparty/g2o/g2o/
 *
 * There is NO CPU fallback: every entry point returns CORB_ERR_NO_DEVICE / CORB_ERR_HIP if the
 * gfx950 device or the kernels are unavailable.
 */
#ifndef CORB_ACCEL_H
#define CORB_ACCEL_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CORB_OK              0
#define CORB_ERR_ARG        -1   /* bad argument / size mismatch with the handle's configuration */
#define CORB_ERR_CAPACITY   -2   /* caller-provided output capacity too small (nothing written past cap) */
#define CORB_ERR_HIP        -3   /* a HIP runtime call failed; see corb_last_error() */
#define CORB_ERR_NO_DEVICE  -4   /* no gfx950 device visible */
#define CORB_ERR_OVERFLOW   -5   /* internal fixed-capacity buffer overflowed (reported, never silent) */
#define CORB_ERR_NUMERIC    -6   /* BA: non-finite values */

const char* corb_last_error(void);          /* thread-local, static storage */
int corb_device_count(void);
int corb_version(void);                     /* 100*major + minor */
/* Layout version of the structs of this header.  CorbBAOptions, CorbBAResult and the record structs carry no size field: a caller checks ONCE, after loading,
   that the library it got was built from the header it was compiled against -- corb_abi_version() == CORB_ABI_VERSION -- and refuses to go on otherwise
   (host/corb_host.hpp: corb::check_abi(); the Python harness does it in load()).  6: the map-point record carries CorbMapPointScratch behind its observation lists (corb_mp_store_record_bytes grew), corb_release_scratch and the
   last two matchers exist; 5: CorbBAResult gained pcg_residual_max / _last / grad_inf;
   4 was round 4's layout (CorbBAOptions 32 bytes with pc_multilevel / scale_factor, CorbBAResult.pc_levels). */
#define CORB_ABI_VERSION 6
int corb_abi_version(void);
/* Page-locked host memory from the HIP runtime THIS library is linked with: host buffers handed to corb_*_upload_batch / corb_*_fetch_batch travel by
 * asynchronous DMA only if that runtime knows them as pinned (a buffer pinned through another copy of the runtime loaded in the same process -- e.g. the
 * one a Python framework ships -- is treated as pageable: staged, synchronous copies). */
int corb_pinned_alloc(size_t bytes, void** out);
int corb_pinned_free(void* p);
/* Optional, once per process and device at start-up: creates the per-device workspace lanes (stream, events, page-locked scratch).  Rounds 1-2 also
 * pre-loaded rocBLAS / rocSOLVER here; the library links neither any more (the dense solves are csrc/dense_chol.hip). */
int corb_warmup(int device);
/* Gives the device and page-locked memory the library keeps between calls on `device` back to the runtime: the bump arenas of its two workspace lanes (they grow to what
 * the largest call needed -- ~9 GB after a 50 000-keyframe global BA -- and never shrink by themselves) and the staging of large host-array BA calls (~0.8 GB + 64 MB
 * page-locked at that size).  What a call of another thread holds at this moment is skipped.  *bytes_released (optional) = what was freed.  The stores are not touched. */
int corb_release_scratch(int device, uint64_t* bytes_released);

/* 28-byte POD, bit-identical to cv::KeyPoint as filled by the reference
 * (C/src/ORBextractor.cc:837-847, 1094-1101): pt, size, angle, response, octave, class_id */
typedef struct CorbKeyPoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} CorbKeyPoint;

/* ============================ ORB extraction ==============================================
 * Replaces ORB_SLAM2::ORBextractor (C/include/ORBextractor.h:45-114, C/src/ORBextractor.cc). */
typedef struct CorbOrbConfig {
    int32_t nfeatures;      /* ORBextractor.nFeatures   (C/src/Tracking.cc:112) */
    float   scale_factor;   /* ORBextractor.scaleFactor (:113) */
    int32_t nlevels;        /* ORBextractor.nLevels     (:114) */
    int32_t ini_th_fast;    /* ORBextractor.iniThFAST   (:115) */
    int32_t min_th_fast;    /* ORBextractor.minThFAST   (:116) */
    int32_t width, height;  /* image size this handle is built for (pyramid geometry is static) */
    int32_t max_images;     /* images processed per launch (1 = one eye, drop-in for operator()) */
    int32_t device;         /* HIP device ordinal */
} CorbOrbConfig;

typedef struct CorbOrb CorbOrb;

/* ORBextractor::ORBextractor (C/src/ORBextractor.cc:410-470) */
int corb_orb_create(const CorbOrbConfig* cfg, CorbOrb** out);
void corb_orb_destroy(CorbOrb* h);

/* ORBextractor::operator() (C/src/ORBextractor.cc:1043-1105), one host image in, host results out.
 * `mask` of the reference is ignored there and absent here.  Empty image (img==NULL or w*h==0)
 * => *n = 0, CORB_OK (mirrors :1046-1047).  Synchronous. */
int corb_orb_extract(CorbOrb* h, const uint8_t* img, int width, int height, int stride,
                     CorbKeyPoint* keypoints, uint8_t* descriptors /* cap x 32 */, int cap, int* n);

/* Getters GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (C/include/ORBextractor.h:62-82) + mnFeaturesPerLevel + umax.
 * Any pointer may be NULL.  Arrays have nlevels entries (umax: 16). */
int corb_orb_tables(const CorbOrb* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                    int32_t* features_per_level, int32_t* umax);

/* mvImagePyramid[level] of image `image` after the last extraction (C/include/ORBextractor.h:85),
 * copied to host with pitch == *width.  dst may be NULL to query the size. blurred!=0 returns the
 * 7x7-Gaussian working copy used for the descriptors (C/src/ORBextractor.cc:1085-1086). */
int corb_orb_pyramid_level(CorbOrb* h, int image, int level, int blurred, uint8_t* dst, size_t dst_bytes,
                           int* width, int* height);

/* Batched, device-resident form of the same operator (the throughput path).
 *   upload : copy one host image into slot `image` (async on the handle's stream; contiguous images take the fast path:
 *            one 1-D copy + a re-pitching kernel -- a strided 2-D copy of a 1241-byte-wide image costs 2.6 ms)
 *   run    : launch the whole pipeline for images [0, n_images) (async).  A run of many images is issued as two part-batches half a pipeline apart (the
 *            second on a side stream of the handle); every call that reads results or rewrites inputs (upload, sync, fetch, ...) joins them first, so to the
 *            caller a run is one asynchronous operation, and back-to-back runs without such a call in between keep the two parts staggered
 *   sync   : wait for everything the handle has enqueued; returns CORB_ERR_OVERFLOW if any image overflowed
 *   fetch  : copy results of one image to host (synchronous) */
int corb_orb_upload(CorbOrb* h, int image, const uint8_t* img, int stride);
int corb_orb_run(CorbOrb* h, int n_images);
int corb_orb_sync(CorbOrb* h);
int corb_orb_fetch(CorbOrb* h, int image, CorbKeyPoint* keypoints, uint8_t* descriptors, int cap, int* n);
/* pre-quadtree candidate list of one level (cell-row-major order, ORBextractor.cc:789-829), for tests */
int corb_orb_fetch_candidates(CorbOrb* h, int image, int level, CorbKeyPoint* out, int cap, int* n);
/* host-buffer batches: n tightly packed images in one copy / all results of n images in one set of copies (pinned host memory = DMA) */
int corb_orb_upload_batch(CorbOrb* h, int first_image, int n_images, const uint8_t* imgs /* n x height x width */);
int corb_orb_capacity(CorbOrb* h);                  /* entries per image of the result arrays */
int corb_orb_fetch_batch(CorbOrb* h, int first_image, int n_images, CorbKeyPoint* keypoints /* [n][capacity] */, uint8_t* descriptors /* [n][capacity][32] */,
                         int32_t* counts /* [n] */);
/* device pointer + pitch of level-0 plane of slot `image` (to fill inputs without a host copy) */
int corb_orb_device_image(CorbOrb* h, int image, void** dptr, size_t* pitch);

/* ============================ stereo front-end =============================================
 * One client's per-frame work in Frame::Frame(stereo) (C/src/Frame.cc:61-117): left + right
 * ORBextractor::operator() and Frame::ComputeStereoMatches (C/src/Frame.cc:470-644), for a batch
 * of `max_frames` stereo frames per launch.  Frame f uses image slots 2f (left) and 2f+1 (right). */
typedef struct CorbStereo CorbStereo;
typedef struct CorbStereoConfig {
    CorbOrbConfig orb;      /* orb.max_images is ignored (= 2*max_frames) */
    int32_t max_frames;
    float fx;               /* Camera.fx */
    float bf;               /* Camera.bf  (Frame::mbf) */
} CorbStereoConfig;

int corb_stereo_create(const CorbStereoConfig* cfg, CorbStereo** out);
void corb_stereo_destroy(CorbStereo* h);
CorbOrb* corb_stereo_orb(CorbStereo* h);           /* the underlying batched extractor (borrowed) */
int corb_stereo_upload(CorbStereo* h, int frame, const uint8_t* left, const uint8_t* right, int stride);
int corb_stereo_run(CorbStereo* h, int n_frames);  /* async: extraction of 2n images + stereo match */
int corb_stereo_sync(CorbStereo* h);
/* whole batches with one copy each way; results strided by corb_orb_capacity(corb_stereo_orb(h)) */
int corb_stereo_upload_batch(CorbStereo* h, int first_frame, int n_frames, const uint8_t* left_right /* per frame: left image, right image */);
int corb_stereo_fetch_matches_batch(CorbStereo* h, int first_frame, int n_frames, float* u_right /* [n][capacity] */, float* depth, int32_t* n_matched /* [n] */);
/* mvuRight / mvDepth of the LEFT keypoints of `frame` (-1 = no match), n = left keypoint count */
int corb_stereo_fetch_matches(CorbStereo* h, int frame, float* u_right, float* depth, int cap, int* n, int* n_matched);

/* ---- the reference's operating point: a client hands over ONE stereo frame at a time (Frame::Frame(stereo), C/src/Frame.cc:61-117, called per frame by
 * Tracking::GrabImageStereo, C/src/Tracking.cc:166-203) ----
 * corb_stereo_frames: n frames (n small: 1, 2, 8 ...) host buffers in, host buffers out, in ONE call: one host-to-device transfer of the 2n images, the
 * kernel chain (replayed as a captured hipGraph per n), one pack kernel, ONE device-to-host transfer, ONE synchronisation.
 *   images : n x {left, right} x height x width bytes, tightly packed
 *   result : n blocks of corb_stereo_frame_layout().frame_bytes bytes; block f (frame f):
 *              int32 n_left, n_right, n_matched, status (0 = ok, else CORB_ERR_OVERFLOW of an image of the frame)
 *              CorbKeyPoint[capacity] left keypoints   at off_kp_left      uint8[capacity][32] left descriptors   at off_desc_left
 *              CorbKeyPoint[capacity] right keypoints  at off_kp_right     uint8[capacity][32] right descriptors  at off_desc_right
 *              float[capacity] mvuRight at off_u_right, float[capacity] mvDepth at off_depth (of the left keypoints, -1 = no match)
 *            only the first n_left / n_right entries of a section are written.
 * Both buffers should be page-locked (corb_pinned_alloc) so that the transfers are DMA; pageable memory works and is slower.
 * timing (may be NULL): device milliseconds of the three stages of this call (costs four event records). */
typedef struct CorbStereoFrameLayout {
    int32_t capacity, frame_bytes;
    int32_t off_kp_left, off_kp_right, off_desc_left, off_desc_right, off_u_right, off_depth;
} CorbStereoFrameLayout;
typedef struct CorbStereoFrameTiming { float ms_upload, ms_kernels, ms_download; } CorbStereoFrameTiming;
int corb_stereo_frame_layout(CorbStereo* h, CorbStereoFrameLayout* out);
int corb_stereo_frames(CorbStereo* h, int n_frames, const uint8_t* images, void* result, CorbStereoFrameTiming* timing);

/* ============================ RGB-D and monocular front-end ===============================
 * One client's per-frame work in Frame::Frame(RGB-D) (C/src/Frame.cc:119-172) and Frame::Frame(monocular) (:174-228) with the input conversions of
 * Tracking::GrabImageRGBD / GrabImageMonocular (C/src/Tracking.cc:206-264), for a batch of `max_frames` frames per launch:
 *   1. colour -> grey as cvtColor RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY (chosen by `rgb` and `channels`; one channel is used as it is)
 *   2. ORBextractor::operator() on the grey image (the handle's extractor, corb_rgbd_orb)
 *   3. Frame::UndistortKeyPoints -> keys_un (mvKeysUn; = keys when k1 == 0)
 *   4. RGB-D: depth at the distorted keypoint, scaled as Mat::convertTo(CV_32F, 1 / DepthMapFactor) does, and Frame::ComputeStereoFromRGBD -> u_right
 *      (mvuRight) and depth (mvDepth), -1 where the depth is not > 0; monocular: both -1
 * Frame f uses image slot f of the extractor.  Input of one frame: the colour image (height x width x channels bytes, tightly packed) followed, for
 * RGB-D, by the depth image (height x width uint16 or float32, tightly packed); corb_rgbd_frame_layout().input_bytes bytes per frame. */
#define CORB_SENSOR_MONOCULAR 0      /* System::MONOCULAR */
#define CORB_SENSOR_RGBD      2      /* System::RGBD */
#define CORB_DEPTH_U16        0      /* depth image CV_16U (TUM's PNGs) */
#define CORB_DEPTH_F32        1      /* depth image CV_32F */
typedef struct CorbRgbd CorbRgbd;
typedef struct CorbCameraConfig {
    CorbOrbConfig orb;                /* max_images is ignored: the handle sizes its extractor to max_frames */
    int32_t max_frames;
    int32_t sensor;                   /* CORB_SENSOR_MONOCULAR / CORB_SENSOR_RGBD */
    int32_t channels;                 /* bytes per input pixel: 1 (grey), 3 (RGB / BGR), 4 (RGBA / BGRA) */
    int32_t rgb;                      /* Camera.RGB: 1 = RGB(A) order, 0 = BGR(A) order (ignored for one channel) */
    float fx, fy, cx, cy;             /* Camera.fx .. Camera.cy */
    float k1, k2, p1, p2, k3;         /* Camera.k1 .. Camera.k3 (k3 = 0: the 4-coefficient model, Tracking.cc:65-75) */
    float bf;                         /* Camera.bf (RGB-D) */
    float depth_map_factor;           /* DepthMapFactor as in the settings file; the handle applies Tracking.cc:141-145 (|.| < 1e-5 -> 1, else 1 / value) */
    int32_t depth_format;             /* CORB_DEPTH_U16 / CORB_DEPTH_F32 (RGB-D) */
} CorbCameraConfig;
int corb_rgbd_create(const CorbCameraConfig* cfg, CorbRgbd** out);
void corb_rgbd_destroy(CorbRgbd* h);
CorbOrb* corb_rgbd_orb(CorbRgbd* h);                 /* the underlying batched extractor (borrowed): corb_orb_pyramid_level, corb_orb_tables ... */
/* frames first .. first+n-1 from ONE contiguous block of n * input_bytes bytes (one copy + one conversion kernel, asynchronous) */
int corb_rgbd_upload_batch(CorbRgbd* h, int first_frame, int n_frames, const uint8_t* input);
int corb_rgbd_run(CorbRgbd* h, int n_frames);        /* async: frames 0 .. n-1: extraction, undistortion, depth */
int corb_rgbd_sync(CorbRgbd* h);                     /* CORB_ERR_OVERFLOW if a frame overflowed an internal buffer */
/* results of frames first .. first+n-1, strided by capacity = corb_orb_capacity(corb_rgbd_orb(h)) per frame: keys / keys_un [n][capacity],
 * desc [n][capacity][32], u_right / depth [n][capacity], counts [n]; any array but counts may be NULL; one synchronisation */
int corb_rgbd_fetch_batch(CorbRgbd* h, int first_frame, int n_frames, CorbKeyPoint* keys, CorbKeyPoint* keys_un, uint8_t* desc, float* u_right, float* depth,
                          int32_t* counts);
/* corb_rgbd_frames: the per-frame call of a client (Tracking::GrabImageRGBD / GrabImageMonocular), like corb_stereo_frames: one host-to-device transfer of
 * the n inputs, the kernel chain (one captured hipGraph per n, one stream), ONE device-to-host transfer of n result blocks, ONE synchronisation.
 *   result : n blocks of frame_bytes bytes; block f: int32 n (keypoints), status (0 = ok, else CORB_ERR_OVERFLOW), then at their offsets
 *            CorbKeyPoint[capacity] mvKeys, CorbKeyPoint[capacity] mvKeysUn, uint8[capacity][32] mDescriptors, float[capacity] mvuRight, float[capacity] mvDepth;
 *            only the first n entries of a section are written.
 * timing (may be NULL): device milliseconds of upload / kernels / download. */
typedef struct CorbRgbdFrameLayout {
    int32_t capacity, frame_bytes, input_bytes;
    int32_t off_keys, off_keys_un, off_desc, off_u_right, off_depth;
} CorbRgbdFrameLayout;
int corb_rgbd_frame_layout(CorbRgbd* h, CorbRgbdFrameLayout* out);
int corb_rgbd_frames(CorbRgbd* h, int n_frames, const uint8_t* input, void* result, CorbStereoFrameTiming* timing);
/* Frame::ComputeImageBounds (C/src/Frame.cc:440-468) of the handle's calibration: out = {mnMinX, mnMaxX, mnMinY, mnMaxY} */
int corb_rgbd_image_bounds(CorbRgbd* h, float out[4]);

/* per-kernel device timing (HIP events on the handle's own stream).  enable, run, sync, then read. */
typedef struct CorbKernelTime {
    char name[48];
    double total_ms;
    int64_t launches;
} CorbKernelTime;
int corb_orb_profile(CorbOrb* h, int enable);   /* 0 off; 1 time every launch of the product sequence (two overlapping half-batches);
                                                    2 as 1 but unsplit on one stream: stand-alone kernel durations */
int corb_orb_profile_read(CorbOrb* h, CorbKernelTime* out, int cap, int* n);   /* resets the accumulators */

/* ============================ descriptor matching ==========================================
 * Replaces the arithmetic of ORB_SLAM2::ORBmatcher (C/include/ORBmatcher.h:41-107). Flat arrays in,
 * indices out; the C++ adapter maps indices back to MapPoint*. Host pointers; synchronous. */

/* ORBmatcher::DescriptorDistance (C/src/ORBmatcher.cc:1792-1808) for n pairs a[i] vs b[i] */
int corb_descriptor_distance(const uint8_t* a, const uint8_t* b, int n, int32_t* dist, int device);

/* DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) flattened: ascending node ids */
typedef struct CorbFeatVec {
    int32_t n_nodes;
    const uint32_t* node_id;
    const int32_t* offset;      /* n_nodes + 1 */
    const uint32_t* idx;        /* feature indices, offset[n_nodes] entries */
} CorbFeatVec;

typedef struct CorbBowSide {
    const uint8_t* desc;        /* n x 32 */
    const float* angle;         /* mvKeysUn[i].angle (only read if check_orientation) */
    const uint8_t* valid;       /* 1 = feature has a non-bad MapPoint (may be NULL for the Frame side) */
    int32_t n;
    CorbFeatVec fv;
} CorbBowSide;

/* variant 0: SearchByBoW(KeyFrame*,Frame&,...) (C/src/ORBmatcher.cc:162-291) and
 *            SearchByBoWInServer (294-423): match[iF] = KF feature index or -1, `match` has b.n entries
 * variant 1: SearchByBoW(KeyFrame*,KeyFrame*,...) (657-790): match[i1] = idx2 or -1, a.n entries
 * Returns the reference's return value (number of matches) in *n_matches. */
int corb_search_by_bow(int variant, const CorbBowSide* a, const CorbBowSide* b, float nnratio,
                       int check_orientation, int32_t* match, int* n_matches, int device);

typedef struct CorbTriSide {
    const uint8_t* desc;        /* n x 32 */
    const CorbKeyPoint* kp;     /* mvKeysUn */
    const float* u_right;       /* mvuRight */
    const uint8_t* has_mappoint;
    int32_t n;
    CorbFeatVec fv;
} CorbTriSide;

/* ORBmatcher::SearchForTriangulation (C/src/ORBmatcher.cc:792-958).  F12 row-major float 3x3;
 * (ex,ey) the epipole of KF1's centre in KF2 (:803-808); scale2/sigma2_2 = pKF2->mvScaleFactors /
 * mvLevelSigma2.  pairs: (idx1, idx2) sorted by idx1, capacity a.n pairs. */
int corb_search_for_triangulation(const CorbTriSide* a, const CorbTriSide* b, const float* F12, float ex, float ey,
                                  const float* scale2, const float* sigma2_2, int nlevels, int only_stereo,
                                  int check_orientation, int32_t* pairs, int* n_matches, int device);

/* ============================ projection-guided matchers (Tracking thread) ================
 * ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)  (C/src/ORBmatcher.cc:45-131, TrackLocalMap) and
 * ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)       (C/src/ORBmatcher.cc:1470-1614, TrackWithMotionModel),
 * including Frame::AssignFeaturesToGrid / GetFeaturesInArea (C/src/Frame.cc:230-245, 331-384).  Both are greedy and order
 * dependent in the reference (a feature can be claimed once); the results here are identical to the sequential order. */
typedef struct CorbFrameView {       /* what the matchers read from the current Frame */
    const CorbKeyPoint* keys_un; const float* u_right; const uint8_t* desc; int32_t n;
    const uint8_t* claimed;          /* mvpMapPoints[i] holds a MapPoint with Observations()>0 */
    float min_x, min_y, max_x, max_y;            /* mnMinX, mnMinY, mnMaxX, mnMaxY */
    const float* scale; int32_t nlevels;         /* mvScaleFactors */
} CorbFrameView;
typedef struct CorbTrackedPoint {    /* MapPoint fields set by Frame::isInFrustum */
    float proj_x, proj_y, proj_xr, view_cos;     /* mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos */
    int32_t level;                   /* mnTrackScaleLevel */
    uint8_t valid;                   /* mbTrackInView && !isBad() */
    uint8_t claims;                  /* Observations()>0 */
    uint8_t pad[2];
} CorbTrackedPoint;
typedef struct CorbLastPoint {       /* one feature of the last frame */
    float world[3];                  /* pMP->GetWorldPos() */
    float angle;                     /* LastFrame.mvKeysUn[i].angle */
    int32_t octave;                  /* LastFrame.mvKeys[i].octave */
    uint8_t valid;                   /* has a MapPoint && !mvbOutlier[i] */
    uint8_t claims;                  /* pMP->Observations()>0 */
    uint8_t pad[2];
} CorbLastPoint;
/* match[i] per current-frame feature = index of the assigned map point / last-frame feature or -1; *n_matches = return value */
int corb_search_by_projection_map(const CorbFrameView* frame, const CorbTrackedPoint* points, const uint8_t* point_desc /* n x 32, pMP->GetDescriptor() */,
                                  int n_points, float th, float nnratio, int32_t* match, int* n_matches, int device);
int corb_search_by_projection_frame(const CorbFrameView* cur, const float* Tcw /* 16, current pose */, const float* Tlw /* 16, last pose */,
                                    float fx, float fy, float cx, float cy, float bf, float mb, const CorbLastPoint* last,
                                    const uint8_t* last_desc /* n x 32, pMP->GetDescriptor() */, int n_last, float th, int mono,
                                    int check_orientation, int32_t* match, int* n_matches, int device);

/* ---- matchers that project MapPoints into a KeyFrame, or into the current Frame for relocalisation ----
 * The adapter evaluates the pointer-level skip tests (NULL / isBad() / sAlreadyFound / IsInKeyFrame / vbAlreadyMatched) into
 * `valid`, and applies the pointer-level consequences of a match (Replace / AddObservation / AddMapPoint) from the returned
 * indices; everything arithmetic (projection, distance and viewing-angle gates, PredictScale, grid search, octave window,
 * chi2 gate, Hamming minimum, rotation histogram) runs on the device. */
typedef struct CorbKeyFrameView {    /* KeyFrame (Fuse, SearchBySim3) or the current Frame (relocalisation) */
    const CorbKeyPoint* keys_un; const float* u_right; const uint8_t* desc; int32_t n;   /* mvKeysUn, mvuRight, mDescriptors */
    float min_x, min_y, max_x, max_y;            /* mnMinX .. mnMaxY */
    const float* scale; const float* inv_level_sigma2; int32_t nlevels;   /* mvScaleFactors, mvInvLevelSigma2 */
    float log_scale_factor;                      /* mfLogScaleFactor */
    float fx, fy, cx, cy, bf;
} CorbKeyFrameView;
typedef struct CorbMapPointView {
    float world[3];                  /* GetWorldPos() */
    float normal[3];                 /* GetNormal() (Fuse) */
    float min_distance, max_distance;/* mfMinDistance, mfMaxDistance (Get*DistanceInvariance() = 0.8f / 1.2f times these) */
    float angle;                     /* relocalisation: pKF->mvKeysUn[i].angle of the keyframe feature holding the point */
    uint8_t valid; uint8_t pad[3];
} CorbMapPointView;
/* int SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12, int windowSize) (C/src/ORBmatcher.cc:540-655): the monocular
 * initialiser's matcher (Tracking::MonocularInitialization, C/src/Tracking.cc:606).  f1 / f2: keys_un, desc, n and (f2) the image bounds are read (u_right, claimed, scale
 * are not).  prev_matched: n(f1) x 2 floats, vbPrevMatched, read and written; matches12[i1] = feature of F2 or -1; nnratio = mfNNratio, check_orientation =
 * mbCheckOrientation; *n_matches = the return value. */
int corb_search_for_initialization(const CorbFrameView* f1, const CorbFrameView* f2, float* prev_matched, int window_size, float nnratio, int check_orientation,
                                   int32_t* matches12, int* n_matches, int device);
/* int SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>& sAlreadyFound, th, ORBdist) (C/src/ORBmatcher.cc:1616-1744).
 * claimed[i] = CurrentFrame.mvpMapPoints[i] holds a MapPoint; match[i] per current-frame feature = point index or -1. */
int corb_search_by_projection_reloc(const CorbKeyFrameView* cur, const uint8_t* claimed, const float* Tcw /* 16 */, const CorbMapPointView* points,
                                    const uint8_t* point_desc /* n x 32 */, int n_points, float th, int orb_dist, int check_orientation,
                                    int32_t* match, int* n_matches, int device);
/* int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th) (C/src/ORBmatcher.cc:425-538;
 * callers: C/src/LoopClosing.cc:377, S/src/GlobalOptimize.cpp:199 -- the last matcher before CorrectLoop / the global BA of a fusion event).
 * claimed[idx] = vpMatched[idx] != NULL on entry (NULL = no feature holds a point); points[i].valid = !pMP->isBad() && !spAlreadyFound.count(pMP);
 * match[idx] per keyframe feature = index of the point this call writes into vpMatched[idx], or -1; *n_matches = the return value. */
int corb_search_by_projection_scw(const CorbKeyFrameView* kf, const uint8_t* claimed, const float* Scw /* 16 */, const CorbMapPointView* points,
                                  const uint8_t* point_desc /* n x 32 */, int n_points, float th, int32_t* match, int* n_matches, int device);
/* int Fuse(KeyFrame*, const vector<MapPoint*>&, th) (:960-1116): sim3 = 0, T = Tcw (16), Ow = pKF->GetCameraCenter();
 * int Fuse(KeyFrame*, cv::Mat Scw, vpPoints, th, vpReplacePoint) (:1118-1241): sim3 = 1, T = Scw (16), Ow ignored.
 * best_idx[i] = keyframe feature into which point i is fused (bestDist <= TH_LOW) or -1; *n_fused = the return value. */
int corb_fuse(const CorbKeyFrameView* kf, const float* T, const float* Ow, int sim3, const CorbMapPointView* points, const uint8_t* point_desc,
              int n_points, float th, int32_t* best_idx, int32_t* best_dist, int* n_fused, int device);
/* int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, s12, R12, t12, th) (:1244-1468).
 * points1[i] / points2[i] = the MapPoint of feature i of KF1 / KF2 (valid = exists, !isBad(), not already matched);
 * match12[i1] = feature of KF2 whose MapPoint becomes vpMatches12[i1], or -1; *n_found = the return value. */
int corb_search_by_sim3(const CorbKeyFrameView* kf1, const CorbKeyFrameView* kf2, const float* T1w, const float* T2w,
                        const CorbMapPointView* points1, const uint8_t* desc1, const CorbMapPointView* points2, const uint8_t* desc2,
                        float s12, const float* R12 /* 9 */, const float* t12 /* 3 */, float th, int32_t* match12, int* n_found, int device);

/* ---- map maintenance next to the hot path ----
 * void MapPoint::ComputeDistinctiveDescriptors() (C/src/MapPoint.cc:337-402) for a batch of map points: desc = the descriptors
 * of every point's non-bad observations stacked in std::map order, point p owns rows offset[p] .. offset[p+1];
 * best_idx[p] = row (relative to offset[p]) the point adopts as mDescriptor, -1 for a point without descriptors. */
int corb_distinctive_descriptors(const uint8_t* desc, const int32_t* offset, int n_points, int32_t* best_idx, int device);
/* void MapFusion::insertServerMapToGlobleMap(ServerMap*, cv::Mat To2n) (S/src/MapFusion.cpp:622-658), arithmetic part: every
 * keyframe pose Tcw <- Tcw * To2n (4x4 row-major, in place), every map point p <- Rwc (p - tcw) with To2n = [Rcw | tcw]. */
int corb_rebase_map(const float* To2n, float* poses, int n_poses, float* points, int n_points, int device);

/* ============================ global bundle adjustment =====================================
 * Replaces the arithmetic of Optimizer::GlobalBundleAdjustemnt -> BundleAdjustment
 * (C/src/Optimizer.cc:43-270) and the g2o pieces it drives: EdgeSE3ProjectXYZ /
 * EdgeStereoSE3ProjectXYZ (G/types/types_six_dof_expmap.{h,cpp}), BlockSolver_6_3 Schur solve
 * (G/core/block_solver.hpp:354-604), Levenberg-Marquardt (G/core/optimization_algorithm_levenberg.cpp).
 * The adapter flattens KeyFrames / MapPoints and applies the nLoopKF write-back policy. */
typedef struct CorbBAEdge {
    int32_t pose, point;
    float u, v, u_right;        /* u_right < 0 : monocular 2-D edge, else stereo 3-D edge */
    float inv_sigma2;           /* pKF->mvInvLevelSigma2[kpUn.octave] */
} CorbBAEdge;

typedef struct CorbBAProblem {
    int32_t n_poses, n_points, n_edges;
    const float* poses;         /* n_poses x 16 row-major Tcw (cv::Mat CV_32F) */
    const uint8_t* pose_fixed;  /* mnId==1 || getFixed() */
    const float* points;        /* n_points x 3 */
    const uint8_t* point_fixed;
    const CorbBAEdge* edges;
    float fx, fy, cx, cy, bf;   /* shared camera, used when intr == NULL (single-client maps) */
    const float* intr;          /* n_poses x 5: fx, fy, cx, cy, bf of EVERY keyframe -- the reference sets them per edge from the observing keyframe
                                   (e->fx = pKF->fx; ... e->bf = pKF->mbf, C/src/Optimizer.cc:160-163, 189-193; KeyFrame.h:68 serialises them per keyframe), so a
                                   fused map of clients with different cameras (KITTI00-02.yaml vs KITTI04-12.yaml) is one problem.  NULL = shared camera above. */
} CorbBAProblem;

typedef struct CorbBAResult {
    float* poses;               /* n_poses x 16 (fixed poses copied through) */
    float* points;              /* n_points x 3 */
    double* chi2;               /* iterations+1 entries: initial, then after each outer iteration (may be NULL) */
    double* lambda;             /* iterations entries (may be NULL) */
    int32_t iters_done;
    int32_t trials_total;
    double ms_total, ms_build, ms_schur, ms_solve, ms_update;   /* device time of the call; the phase times are measured from 65 536 observations on (0 below) */
    int32_t solver_used;        /* 1 dense Cholesky (csrc/dense_chol.hip; inside the one-workgroup optimiser for small problems), 2 block-sparse PCG,
                                   3 fused single-pose kernel (6x6 LDL^T on the device) */
    int32_t pcg_iterations;     /* total CG iterations over all LM trials */
    /* structure of the last optimize() call (sizes behind the roofline figures of bench.py) */
    int32_t free_poses, free_points, active_edges;
    int64_t nnz_blocks;         /* 6x6 blocks of the reduced camera system, both triangles (0 for the fused small-problem kernel) */
    int64_t schur_pairs;        /* (edge, edge) pairs of the Schur complement = sum over the upper blocks of their co-observed landmarks */
    int32_t pc_block;           /* poses per block of the block-Jacobi preconditioner actually used (PCG) */
    int32_t pc_levels;          /* coarse levels of the multilevel preconditioner (0 = block Jacobi only) */
    /* self-certification of a call that took the PCG solver (CORB_ABI_VERSION >= 5).  g2o's reduced solve is an exact factorisation
       (G/solvers/linear_solver_eigen.h:94-124: residual at rounding level); the iterative solve reports what it reached instead: */
    double pcg_residual_max;    /* largest TRUE relative residual |b - S x| / |b| over the call's reduced solves, recomputed in FP64 by an independent kernel
                                   after each solve (not the recurrence's residual); 0 when no PCG solve ran */
    double pcg_residual_last;   /* the same of the last solve */
    double grad_inf;            /* |J' Omega r|_inf (poses and map points) of a linearisation at the returned estimates; < 0: not computed (dense / small paths) */
    int32_t pcg_refined_trials; /* default tolerance policy (CorbBAOptions.pcg_tol == 0): LM trials whose solve was continued from 1e-6 to 1e-8 before the trial was decided */
    int32_t reserved0;          /* staged calls (corb_ba_solve_staged, corb_local_ba_store): 1 = the window was flattened, optimised and classified on the device,
                                   0 = the host flattening ran -- same results; informational */
} CorbBAResult;

/* linear solver for the reduced camera system (replaces g2o::LinearSolverEigen, G/solvers/linear_solver_eigen.h:94-124) */
typedef struct CorbBAOptions {
    int32_t solver;             /* 0 auto (dense up to 256 free poses -- up to 16 free poses and 2 048 observations the whole optimisation runs in one
                                   workgroup with its own in-LDS Cholesky, above that the blocked Cholesky of dense_chol.hip --, PCG above 256; staged problems with ONE free pose and fixed points:
                                   the fused single-workgroup kernel), 1 dense Cholesky, 2 block-sparse PCG, 3 fused single-pose kernel */
    double  pcg_tol;            /* relative residual |r|/|b| at which CG stops.  > 0: that tolerance for every solve of the call.  0 (default): 1e-8 on problems of up to 256
                                   free keyframes; above, a forcing sequence -- 1e-6 in the first iteration, then clamp(1e-2 x the previous iteration's relative chi2 gain,
                                   1e-8, 1e-6) -- and a trial whose accept / reject decision or lambda factor could depend on the accuracy of its solve (rho near 0, in the
                                   steep part 0.80 .. 0.97 of the lambda schedule, or a predicted decrease below 3e-6 chi2) has the SAME solve continued to 1e-8 before it is
                                   decided.  chi2 after every iteration within 5e-8 relative of a 1e-13 solve on 320 ... 20 000 keyframes (the parity bar is 1e-4; what sets
                                   1e-6 is lambda: see csrc/corb_ba.cpp BAChoice) -- profiles/r05_pcg_tol_sweep.txt */
    int32_t pcg_max_iter;       /* default 4000; not converged => the LM trial is rejected like a failed factorisation */
    int32_t pc_block;           /* poses per block of the block-Jacobi preconditioner: 0 = auto (1 below 128 free poses, 16 above), 1 = the 6x6 diagonal blocks, 8 or 16
                                   (dense diagonal blocks inverted on every 3rd accepted LM trial and after a rejected one) */
    int32_t pc_multilevel;      /* coarse levels next to the 16-pose blocks (linear hats over the keyframe order, stride 8 then 4, Galerkin matrices, block Jacobi per level:
                                   csrc/ba_multilevel.h): 0 = auto (on from 256 free poses: every map the PCG solver takes by default), 1 = off, 2 = on (needs pc_block 16 or auto with >= 128 free poses) */
    float   scale_factor;       /* corb_ba_solve_store with loop_kf == 0 only: ORBextractor's scaleFactor (1.2 in every reference yaml).  > 0: SetWorldPos is followed by
                                   MapPoint::UpdateNormalAndDepth on the records (see corb_ba_solve_store); 0 (default): normal / min_distance / max_distance are left alone.
                                   (The field fills what was padding: sizeof(CorbBAOptions) is unchanged.) */
} CorbBAOptions;

/* optimizer.optimize(nIterations) with bRobust / pbStopFlag semantics of Optimizer.cc:54-270 */
int corb_ba_solve(const CorbBAProblem* problem, int iterations, int robust, volatile int* stop_flag,
                  CorbBAResult* result, int device);
int corb_ba_solve_ex(const CorbBAProblem* problem, int iterations, int robust, volatile int* stop_flag,
                     CorbBAResult* result, int device, const CorbBAOptions* options /* NULL = defaults */);

/* corb_ba_solve_ex with the graph flattening done ON THE DEVICE (the path corb_ba_solve_store takes: ba_flatten.hip) instead of on the host: the host arrays are
 * uploaded as they are, grouped by map point, and indexed / sorted / patterned by kernels.  Same lists as the host flattening, element for element (the tests
 * compare the two); a caller with host arrays has no reason to prefer it except at the largest sizes, where it saves the host-side list building. */
int corb_ba_solve_devflat(const CorbBAProblem* problem, int iterations, int robust, CorbBAResult* result, int device, const CorbBAOptions* options);

/* The dense solver of the reduced camera system on its own (what g2o::LinearSolverEigen / LinearSolverDense do for a dense block matrix,
 * G/solvers/linear_solver_eigen.h:94-124): A x = b for a symmetric positive definite n x n matrix (row-major, only the lower triangle is read), hand-written
 * blocked Cholesky on the FP64 matrix cores (csrc/dense_chol.hip).  Host pointers; *info = 0 or 1 + the first column whose pivot is not positive (x is then
 * meaningless).  Exposed for tests and for adapters with their own small dense systems. */
int corb_spd_solve(const double* A, int n, const double* b, double* x, int* info, int device);

/* TEST AIDS on the two workspace lanes of a device (lane 0: the per-frame calls and corb_spd_solve; lane 1: every bundle adjustment and the essential graph).  Every call
 * that takes a lane bump-allocates its device scratch from the lane's arena and starts at the same base address as the call before it, so it finds that call's leftovers;
 * the rule the library keeps is that a call reads no byte of the arena, of the lane's page-locked staging or of its 4 KB page-locked block that it has not written itself.
 * These three functions let a test put a lane into a chosen dirty state and look at it afterwards.  They take the lane's mutex and are no part of any call's work; a client
 * has no use for them.
 *   fill:   the arena becomes ONE chunk of max(min_bytes, its current total capacity) bytes; every 32-bit word of it, of the staging (if there is one) and of the
 *           page-locked block is set to `word`; synchronises; *capacity (optional) = the chunk's size.  If the chunk cannot be allocated the call fails and leaves
 *           the arena empty, as corb_release_scratch does.
 *   report: *capacity = the arena's total bytes, *n_chunks = its chunks (0 after corb_release_scratch, > 1 never between calls), *staging_capacity = the staging's bytes.
 *   read:   `bytes` bytes at `offset` of the single chunk into `out`; CORB_ERR_ARG if the arena is not exactly one chunk or the range leaves it. */
int corb_scratch_fill(int device, int lane, uint32_t word, uint64_t min_bytes, uint64_t* capacity);
int corb_scratch_report(int device, int lane, uint64_t* capacity, int* n_chunks, uint64_t* staging_capacity);
int corb_scratch_read(int device, int lane, uint64_t offset, uint64_t bytes, void* out);

/* One optimize() call plus the outlier test that follows it.  Sequences of stages express
 *   Optimizer::LocalBundleAdjustment (C/src/Optimizer.cc:487-838): {5, robust, 5.991, 7.815, check_depth=1},
 *                                                                   {10, non-robust, 5.991, 7.815, check_depth=1, allow_reactivate=1}
 *                                     (the final "Check inlier observations" pass tests EVERY edge, also those switched off after the first round, with its
 *                                      last computed chi2 and a fresh depth, :763-790).  pbStopFlag: raised before the first optimize() -> outputs = inputs, no
 *                                      outliers (:706-708); raised later -> the remaining optimize() calls are skipped and the LAST stage's test is applied
 *                                      (bDoMore = false skips only the second round, :712-716).
 *   Optimizer::PoseOptimization     (C/src/Optimizer.cc:272-485): 4 x {10, robust (last: non-robust), 5.991, 7.815,
 *                                     recompute_inactive=1, allow_reactivate=1, reset_estimates=1, float_compare=1}
 * chi2 of an ACTIVE edge is the value of its last computeError() inside optimize() (g2o does not refresh it afterwards;
 * after a rejected last trial it belongs to the rejected state) -- reproduced here; depth is evaluated fresh. */
typedef struct CorbBAStage {
    int32_t iterations, robust;
    float chi2_mono, chi2_stereo;
    int32_t check_depth;            /* edge also becomes an outlier if depth <= 0 (isDepthPositive) */
    int32_t recompute_inactive;     /* computeError() on inactive edges before the test */
    int32_t allow_reactivate;       /* inactive edges may become active (inlier) again */
    int32_t reset_estimates;        /* restart from the input estimates */
    int32_t float_compare;          /* `const float chi2 = e->chi2()` comparison */
    float huber_mono, huber_stereo; /* Huber deltas, (float)sqrt(5.991) / (float)sqrt(7.815) in both callers */
} CorbBAStage;
/* edge_outlier[n_edges]: 1 = classified outlier after the last stage (vToErase / mvbOutlier).  Vertices that never had an
 * active edge are passed through unchanged. */
int corb_ba_solve_staged(const CorbBAProblem* problem, const CorbBAStage* stages, int n_stages, volatile int* stop_flag,
                         CorbBAResult* result, uint8_t* edge_outlier, int device, const CorbBAOptions* options);

/* int Optimizer::PoseOptimization(Frame* pFrame) (C/src/Optimizer.cc:272-485) for a BATCH of frames (the tracking threads of
 * many clients): per frame the 4 x 10 Levenberg-Marquardt rounds with re-classification of the observations between the
 * rounds run inside ONE workgroup without host round trips.  Per observation i of a frame: pMP->GetWorldPos(),
 * mvKeysUn[i].pt, mvuRight[i] (< 0 = monocular edge), mvInvLevelSigma2[octave]. */
typedef struct CorbPoseOptFrame {
    const float* Tcw;           /* 4x4 row-major start pose (pFrame->mTcw) */
    int32_t n_obs;
    const float* points;        /* n_obs x 3 */
    const float* u; const float* v; const float* u_right;
    const float* inv_sigma2;
    float fx, fy, cx, cy, bf;
} CorbPoseOptFrame;
/* Tcw_out: n_frames x 16 (pFrame->SetPose); outlier[f] (may be NULL): n_obs flags = pFrame->mvbOutlier; n_inliers[f] =
 * nInitialCorrespondences - nBad (the function's return value) */
int corb_pose_optimization_batch(const CorbPoseOptFrame* frames, int n_frames, float* Tcw_out, uint8_t* const* outlier,
                                 int32_t* n_inliers, int device);

/* int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, float th2, bool bFixScale)
 * (C/src/Optimizer.cc:1119-1311) for a batch of loop-closure candidates, one workgroup each: optimize(5), chi2 classification,
 * optimize(5 or 10), final classification -- with g2o's numeric Jacobians (delta 1e-9) of EdgeSim3ProjectXYZ /
 * EdgeInverseSim3ProjectXYZ, Huber(sqrt(th2)), LinearSolverDense.  Per correspondence i of a candidate: P3D1c = R1w*P3D1w+t1w and
 * P3D2c (camera-frame points as the adapter already computes them), the two undistorted keypoints, mvInvLevelSigma2 of their octaves. */
typedef struct CorbSim3Problem {
    int32_t n;
    const float* p1c; const float* p2c;              /* n x 3 */
    const float* obs1; const float* obs2;            /* n x 2 */
    const float* inv_sigma2_1; const float* inv_sigma2_2;
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;    /* pKF1->mK, pKF2->mK */
} CorbSim3Problem;
/* R12 (n_problems x 9, row-major), t12 (x 3), s12: g2oS12 in / out (unchanged for a candidate that keeps fewer than 10 correspondences
 * after the first round; its n_inliers is 0).  removed[f][i] = 1: vpMatches1[idx] is nulled.  n_inliers[f] = the return value. */
int corb_optimize_sim3(const CorbSim3Problem* problems, int n_problems, double* R12, double* t12, double* s12, float th2, int fix_scale,
                       uint8_t* const* removed, int32_t* n_inliers, int32_t* iterations /* may be NULL */, int device);

/* void Optimizer::OptimizeEssentialGraph(Cache*, KeyFrame* pLoopKF, KeyFrame* pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)
 * (C/src/Optimizer.cc:840-1117).  The adapter builds the graph exactly as lines 866-1037 do: one g2o::Sim3 per non-bad keyframe
 * (S = quaternion x y z w, translation, scale; CorrectedSim3 value or Sim3(Rcw, tcw, 1)), fixed = (pKF == pLoopKF || getFixed()), and per
 * EdgeSim3 the pair (vertex 0 = vi, vertex 1 = vj) with its measurement Sji = Sjw * Swi.  The library runs optimize(iterations = 20) with
 * lambda_init 1e-16 (numeric Jacobians, identity information), then the SE3 recovery Tiw = [R | t/s] (Tiw_out, K x 16, may be NULL) and the
 * map point correction p <- correctedSwr.map(Srw.map(p)) for points whose reference keyframe index point_ref[m] >= 0 (in place).
 * S is updated in place; chi2_hist (iterations + 1, may be NULL); *iters_done optional. */
int corb_optimize_essential_graph(int n_keyframes, double* S, const uint8_t* fixed, int n_edges, const int32_t* vi, const int32_t* vj,
                                  const double* measurement, int iterations, int fix_scale, float* Tiw_out, int n_points,
                                  const int32_t* point_ref, float* points, double* chi2_hist, int32_t* iters_done, int device);

/* ============================ device-resident keyframe store + map push =====================
 * What the reference serialises per KeyFrame for the client -> server push (C/include/KeyFrame.h:59-87: mnId, mvKeys / mvKeysUn, mDescriptors, mvuRight,
 * mvDepth, mBowVec / mFeatVec ...; boost text archives through ROS services every 6 s, C/src/Cache.cc:322-375, C/src/DataDriver.cc:135-193) kept as one
 * fixed-size SoA record per keyframe IN DEVICE MEMORY: 28-byte keypoints, 32-byte descriptors, mvuRight, mvDepth, the keypoint angles, the "has a good
 * MapPoint" flags and the DBoW2 FeatureVector groups.  A slot is filled device-to-device from the stereo front-end's results (no host trip), matched
 * against other slots without uploads, and pushed to the server rank with RCCL send / receive on the device buffers (one process per GPU over xGMI). */
typedef struct CorbKfStore CorbKfStore;
int corb_kf_store_create(int device, int capacity_keyframes, int max_features, CorbKfStore** out);
void corb_kf_store_destroy(CorbKfStore* s);
int corb_kf_store_record_bytes(const CorbKfStore* s);                 /* bytes of one slot record (what a push moves per keyframe) */
/* slot <- left keypoints / descriptors / mvuRight / mvDepth of frame `frame` of a stereo front-end after corb_stereo_run (device-to-device, asynchronous on
 * the front-end's stream; the store's later calls wait for it) */
int corb_kf_store_put_from_stereo(CorbKfStore* s, int slot, CorbStereo* sf, int frame, uint64_t keyframe_id);
/* slot <- mvKeysUn / descriptors / mvuRight / mvDepth of frame `frame` of an RGB-D / monocular front-end after corb_rgbd_run or corb_rgbd_frames (device-to-device,
 * asynchronous on the front-end's stream, like corb_kf_store_put_from_stereo) */
int corb_kf_store_put_from_rgbd(CorbKfStore* s, int slot, CorbRgbd* h, int frame, uint64_t keyframe_id);
/* slot <- host arrays (adapters / tests); any pointer except kp / desc may be NULL (u_right, depth default to -1) */
int corb_kf_store_put_host(CorbKfStore* s, int slot, const CorbKeyPoint* kp, const uint8_t* desc, const float* u_right, const float* depth, int n, uint64_t keyframe_id);
/* the parts the host computes: DBoW2 FeatureVector (Frame::ComputeBoW, C/src/Frame.cc:397-406) and the per-feature "vpMapPoints[i] && !isBad()" flags
 * (corb_kf_store_compute_bow, last section, computes the FeatureVector on the device from the record's descriptors instead) */
int corb_kf_store_set_bow(CorbKfStore* s, int slot, const CorbFeatVec* fv);
int corb_kf_store_set_flags(CorbKfStore* s, int slot, const uint8_t* has_good_mappoint /* n entries, NULL = all 0 */);
/* slot -> host (any output may be NULL; *n = feature count); fv arrays need max_features (+1 for the offsets) entries */
int corb_kf_store_get(CorbKfStore* s, int slot, CorbKeyPoint* kp, uint8_t* desc, float* u_right, float* depth, uint8_t* flags, int cap, int* n, uint64_t* keyframe_id,
                      uint32_t* fv_node_id, int32_t* fv_offset, uint32_t* fv_idx, int32_t* fv_n_nodes);
/* corb_search_by_bow on two slots (possibly of two stores on the same device): nothing is uploaded but the short list of common vocabulary nodes.
 * variant 0: match has n(slot_b) entries, variant 1: n(slot_a) entries (see corb_search_by_bow). */
int corb_search_by_bow_slots(int variant, CorbKfStore* a, int slot_a, CorbKfStore* b, int slot_b, float nnratio, int check_orientation,
                             int32_t* match, int* n_matches);
/* corb_search_for_triangulation on two slots (has_mappoint = the slots' flags) */
int corb_search_for_triangulation_slots(CorbKfStore* a, int slot_a, CorbKfStore* b, int slot_b, const float* F12, float ex, float ey,
                                        const float* scale2, const float* sigma2_2, int nlevels, int only_stereo, int check_orientation,
                                        int32_t* pairs, int* n_matches);

/* ---- the rest of the push payload: poses, intrinsics, per-feature map points (KeyFrame.h:65-79) and the MapPoint records (MapPoint.h:52-72) ---- */
#define CORB_KF_BAD    1u        /* mbBad */
#define CORB_KF_FIXED  2u        /* ifFixed (Cache.cc:482: entities received from the server) */
#define CORB_MP_BAD    1u
#define CORB_MP_FIXED  2u
#define CORB_NO_MAP_POINT 0xFFFFFFFFFFFFFFFFull
typedef struct CorbKeyFrameMeta {       /* header of a keyframe record */
    uint64_t id;                        /* mnId (globally unique: client c counts from (c-1)*1000000+1, KeyFrame.cc:49) */
    int32_t client_id;                  /* mnClientId */
    uint32_t flags;                     /* CORB_KF_BAD | CORB_KF_FIXED */
    float fx, fy, cx, cy, bf;           /* fx, fy, cx, cy, mbf */
    int32_t nlevels;                    /* mnScaleLevels */
    float Tcw[16];                      /* Tcw, row-major 4x4 */
    float TcwGBA[16];                   /* mTcwGBA */
    uint64_t ba_global_for_kf;          /* mnBAGlobalForKF */
    float inv_level_sigma2[16];         /* mvInvLevelSigma2 */
} CorbKeyFrameMeta;
int corb_kf_store_set_meta(CorbKfStore* s, int slot, const CorbKeyFrameMeta* meta);      /* also sets the record's id */
/* corb_kf_store_put_host + corb_kf_store_set_meta as ONE upload and one synchronisation: a tracked Frame enters its record (per-frame use: corb_track_*) */
int corb_kf_store_put_frame(CorbKfStore* s, int slot, const CorbKeyPoint* kp, const uint8_t* desc, const float* u_right, const float* depth, int n, const CorbKeyFrameMeta* meta);
int corb_kf_store_get_meta(CorbKfStore* s, int slot, CorbKeyFrameMeta* meta);
/* mvpMapPoints as ids (LightMapPoint::mnMapPointId, KeyFrame.h:78): n(slot) entries, CORB_NO_MAP_POINT = none */
int corb_kf_store_set_map_points(CorbKfStore* s, int slot, const uint64_t* mp_id);
int corb_kf_store_get_map_points(CorbKfStore* s, int slot, uint64_t* mp_id, int cap);

/* slots first .. first+n <- n keyframes from host arrays in ONE upload and ONE kernel (adapters that flatten a whole map, benches): meta[n]; the features of
 * keyframe i are entries feat_offset[i] .. feat_offset[i+1] of kp / desc / u_right / depth / mp_id (desc, u_right, depth, mp_id may be NULL: zero descriptors,
 * -1, -1, CORB_NO_MAP_POINT).  Flags and BoW groups of the slots are cleared like corb_kf_store_put_host does. */
int corb_kf_store_put_batch(CorbKfStore* s, int first, int n, const CorbKeyFrameMeta* meta, const int32_t* feat_offset, const CorbKeyPoint* kp, const uint8_t* desc,
                            const float* u_right, const float* depth, const uint64_t* mp_id);

typedef struct CorbMapPointRecord {     /* header of a map-point record; the observations follow it in the record */
    uint64_t id;                        /* mnId */
    uint64_t ref_kf_id;                 /* mpRefKF->mnId */
    uint8_t descriptor[32];             /* mDescriptor; byte offset 16: the kernels read it as four aligned 64-bit words */
    int32_t client_id;                  /* mnClientId */
    int32_t n_obs;                      /* mObservations.size() */
    uint32_t flags;                     /* CORB_MP_BAD | CORB_MP_FIXED */
    float world_pos[3];                 /* mWorldPos */
    float normal[3];                    /* mNormalVector */
    float min_distance, max_distance;   /* mfMinDistance, mfMaxDistance */
    float pos_gba[3];                   /* mPosGBA */
    uint64_t ba_global_for_kf;          /* mnBAGlobalForKF */
} CorbMapPointRecord;                   /* 112 bytes; this is also the on-wire record of corb_map_push_ex */
typedef struct CorbMpStore CorbMpStore;
/* one fixed-size record per MapPoint in device memory: the header above + up to max_observations (keyframe id, feature index) pairs = mObservations */
int corb_mp_store_create(int device, int capacity_points, int max_observations, CorbMpStore** out);
void corb_mp_store_destroy(CorbMpStore* s);
int corb_mp_store_record_bytes(const CorbMpStore* s);
/* slots first .. first+n <- host records; the observations of record i are obs_kf_id / obs_feature_idx [obs_offset[i] .. obs_offset[i+1]) in mObservations order
 * (ascending keyframe id).  A record with more than max_observations observations => CORB_ERR_CAPACITY, nothing written. */
int corb_mp_store_put_host(CorbMpStore* s, int first, int n, const CorbMapPointRecord* records, const int32_t* obs_offset, const uint64_t* obs_kf_id, const uint32_t* obs_feature_idx);
/* slots -> host: records[n], and (optional) the observations padded to max_observations per record: obs_kf_id / obs_feature_idx [n][max_observations] */
int corb_mp_store_get(CorbMpStore* s, int first, int n, CorbMapPointRecord* records, uint64_t* obs_kf_id, uint32_t* obs_feature_idx);

/* RCCL communicator of the client / server ranks (one process per GPU).  Rank 0 of the job calls corb_comm_unique_id and hands the 128 bytes to every rank
 * by its own means (torch.distributed broadcast, a ROS parameter, a file); every rank then calls corb_comm_create.  librccl.so is loaded on first use
 * (its version is checked: the ncclDataType_t constants used here are those of RCCL 2.x). */
typedef struct CorbComm CorbComm;
int corb_comm_unique_id(void* id128);
int corb_comm_create(const void* id128, int rank, int world, int device, CorbComm** out);
/* The same communicator interface over an in-process transport: `world` handles that share a mailbox, each to be driven by its own host thread; records
 * travel as device-to-device copies.  For servers that run several clients' stores in one process, and for exercising the N-rank push on one GPU.
 * devices: [world] HIP device of every rank, NULL = all on device 0. */
int corb_comm_create_local(int world, const int* devices, CorbComm** out /* [world] */);
void corb_comm_destroy(CorbComm* c);
int corb_comm_rank(const CorbComm* c);
int corb_comm_world(const CorbComm* c);

/* Map push (replaces the insertKeyFrameToMap / insertMapPointToMap service batches, C/src/DataDriver.cc:135-193, S/src/MapFusion.cpp:31-190): every rank
 * calls it collectively; rank r sends the keyframe records kf_slots[0..n_kf) and the map-point records mp_slots[0..n_mp) of its stores to `root`, which
 * files the records of rank r in its own stores from kf_dst_first[r] / mp_dst_first[r] on (rank order, its own included).
 * The call is collective-safe: every rank first contributes a header (its local argument verdict, counts, record sizes) to an all-gather; the root checks
 * capacity and placement with corb_map_push_plan and its verdict travels in a second all-gather, so on ANY rank's error EVERY rank returns the same
 * error code before a single record is sent -- no rank is left waiting in a send.  Records travel as one message per rank and store (a rank's selected
 * records are packed into a contiguous staging buffer first, so source and destination slots of the root may overlap). */
typedef struct CorbMapPush {
    CorbKfStore* kf; const int32_t* kf_slots; int32_t n_kf;
    CorbMpStore* mp; const int32_t* mp_slots; int32_t n_mp;          /* mp may be NULL on every rank: keyframes only */
    const int32_t* kf_dst_first; const int32_t* mp_dst_first;        /* root: [world] */
    int32_t* kf_recv_counts; int32_t* mp_recv_counts;                /* root, optional: [world] */
} CorbMapPush;
int corb_map_push_ex(CorbComm* c, const CorbMapPush* push, int root);
/* keyframes only (round 2's signature) */
int corb_map_push(CorbComm* c, CorbKfStore* s, const int* slots, int n_slots, int root, const int* dst_first, int* recv_counts);
/* The push's bookkeeping as a pure function (no device, no communicator; callable on a CPU-only box): what every rank contributed to the header
 * all-gather -> the verdict every rank returns.  CORB_OK, or: a rank's local status != 0 => that status; record sizes differ from the root's =>
 * CORB_ERR_ARG; a destination range outside the root's capacity => CORB_ERR_CAPACITY; two ranks' destination ranges overlap => CORB_ERR_ARG.
 * *failing_rank = the first rank the verdict is about (-1 if none). */
typedef struct CorbPushHeader { int32_t status, n_kf, n_mp, kf_record_bytes, mp_record_bytes; } CorbPushHeader;
int corb_map_push_plan(int world, int root, const CorbPushHeader* headers /* [world] */, int kf_capacity, int mp_capacity,
                       const int32_t* kf_dst_first, const int32_t* mp_dst_first, int* failing_rank);

/* The messages of a push as pure arithmetic on the gathered headers (CPU-testable; what corb_map_push_ex / corb_map_push_begin post): rank `rank` SENDS one message
 * per store with records to `root` (kind 0 = keyframes, 1 = map points; first_record = 0: the packed staging buffer), the root RECEIVES one per rank and store into
 * its slots from kf_dst_first[r] / mp_dst_first[r] on (first_record = that slot), in rank order, keyframes before map points -- the order in which the sender
 * posted them: messages between a pair of ranks match in posting order.  sends / recvs: room for 2 / 2 * world entries.  Returns CORB_OK or CORB_ERR_ARG. */
typedef struct CorbPushMsg { int32_t peer, kind, first_record, n_records; int64_t bytes; } CorbPushMsg;
int corb_map_push_messages(int world, int rank, int root, const CorbPushHeader* headers /* [world] */, const int32_t* kf_dst_first, const int32_t* mp_dst_first,
                           CorbPushMsg* sends, int* n_sends, CorbPushMsg* recvs, int* n_recvs);
/* the four RCCL entry points the record exchange calls (signatures of ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd with comm / stream as void*).
 * corb_comm_test_rccl_exchange runs the exchange's posting loop on a caller-supplied table (a recording fake: no GPU, no librccl) -- the unit test of the RCCL
 * branch's ordering, sizes and error path (a failing send still closes the group). */
typedef struct CorbRcclFns {
    int (*group_start)(void); int (*group_end)(void);
    int (*send)(const void* buf, size_t count, int datatype, int peer, void* comm, void* stream);
    int (*recv)(void* buf, size_t count, int datatype, int peer, void* comm, void* stream);
} CorbRcclFns;
int corb_comm_test_rccl_exchange(const CorbRcclFns* fns, const CorbPushMsg* sends, int n_sends, const CorbPushMsg* recvs, int n_recvs);

/* Asynchronous push.  corb_map_push_setup (collective, once): the root's stores' capacities / record sizes and its destination table travel to every rank, so that
 * afterwards EVERY rank can evaluate corb_map_push_plan itself.  corb_map_push_begin (collective): ONE all-gather of the headers (the only host synchronisation),
 * the same verdict on every rank without a second round, the records packed into the communicator's own staging buffers (grown on demand, never freed per push)
 * and the messages ENQUEUED on the communicator's stream; it returns without waiting for the transfer, which overlaps whatever the caller does next (tracking
 * runs on other streams).  The records of the pushed slots and the root's destination slots must not be touched until corb_map_push_wait (collective-free: every rank
 * waits for its own event) has returned; it finishes the root's bookkeeping (recv counts, stale host copies).  One push in flight per communicator.
 * Exclusion contract: every push locks a rank's stores while its records are packed and posted (a blocking RCCL push: until they have arrived; the in-process
 * transport: the receiving rank also while it copies them in), so a concurrent corb_ba_solve_store / corb_rebase_map_store / corb_track_* call on the same stores
 * sees records either before or after those phases.  Between corb_map_push_begin and corb_map_push_wait NO lock is held -- the transfer is in flight on the device:
 * a call that reads the root's destination slots in that window can see half-received records, and one that rewrites pushed slots can corrupt the message.  Keeping
 * the stores still in that window is the caller's job, as with the buffers of any asynchronous collective. */
int corb_map_push_setup(CorbComm* c, int root, CorbKfStore* kf, CorbMpStore* mp, const int32_t* kf_dst_first /* root: [world] */, const int32_t* mp_dst_first /* root: [world] or NULL */);
int corb_map_push_begin(CorbComm* c, const CorbMapPush* push, int root);
int corb_map_push_wait(CorbComm* c);

/* Server side of a push, on records: MapFusion::insertServerMapToGlobleMap (S/src/MapFusion.cpp:622-658; also :64-66, :126-131 for late arrivals):
 * Tcw <- Tcw * To2n for the keyframe slots, p <- Rwc (p - tcw) for the map-point slots, in place in device memory. */
int corb_rebase_map_store(const float* To2n, CorbKfStore* kf, const int32_t* kf_slots, int n_kf, CorbMpStore* mp, const int32_t* mp_slots, int n_mp);

/* Optimizer::GlobalBundleAdjustemnt / BundleAdjustment (C/src/Optimizer.cc:43-270) on store records -- what the server rank runs after a push + re-basing
 * (S/src/GlobalOptimize.cpp:444): vertices = the non-bad keyframes kf_slots (fixed iff mnId == 1 or CORB_KF_FIXED, :84-98) and the non-bad map points
 * mp_slots (:106-121); edges = every observation (keyframe id, feature) of those points whose keyframe is among kf_slots and not bad (:123-196), stereo iff
 * mvuRight[feature] >= 0, information mvInvLevelSigma2[octave]; intrinsics per keyframe.  The graph is built on the device from the records (no host
 * flattening, no uploads); results are written back into the records as the reference does (:216-262): loop_kf == 0 -> Tcw / world_pos, else TcwGBA /
 * pos_gba and ba_global_for_kf = loop_kf.  result->poses (n_kf x 16) / points (n_mp x 3) are optional copies (NULL = none).
 * loop_kf == 0: the reference follows SetWorldPos with pMP->UpdateNormalAndDepth() (:254-256).  With options->scale_factor > 0 the write-back does the same on the
 * records -- normal, min_distance, max_distance from the observers that are vertices of this solve (a global BA holds every keyframe of the map: all of them), with
 * the poses the solve left and mvScaleFactors rebuilt from scale_factor as ORBextractor.cc:418-424 does -- so that tracking calls (corb_track_search_local_points'
 * isInFrustum) can run on the records at once.  With scale_factor == 0 the three fields are left alone and the caller refreshes them (the adapter's
 * ReadBackMapPoints calls UpdateNormalAndDepth on the object) and re-files the points. */
int corb_ba_solve_store(CorbKfStore* kf, const int32_t* kf_slots, int n_kf, CorbMpStore* mp, const int32_t* mp_slots, int n_mp,
                        int iterations, int robust, volatile int* stop_flag, uint64_t loop_kf, CorbBAResult* result, const CorbBAOptions* options);

/* void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Cache* pCache) (C/src/Optimizer.cc:487-838) on store records -- what LocalMapping
 * runs after every keyframe (C/src/LocalMapping.cc:79).  The caller selects the window as the reference does (:493-546) and passes it as slots:
 *   kf_slots[0 .. n_local)     lLocalKeyFrames: free unless mnId == 1 or CORB_KF_FIXED (:569)
 *   kf_slots[n_local .. n_kf)  lFixedCameras: fixed (:582)
 *   mp_slots                   lLocalMapPoints (fixed iff CORB_MP_FIXED, :620)
 * Edges = every observation of those points in one of those keyframes (:626-700), built on the device from the records as for corb_ba_solve_store.
 * stages = the optimize(5) / "Check inlier observations" / optimize(10) schedule as CorbBAStage entries (the same two stages the host-pointer form
 * corb_ba_solve_staged is given for LocalBundleAdjustment); stop_flag = pbStopFlag with the reference's semantics (raised before the call: nothing is touched).
 * Afterwards, on the records (:760-836):
 *   apply_erase != 0: vToErase -- for every outlier observation the keyframe record's map-point id of that feature <- CORB_NO_MAP_POINT
 *     (pKFi->EraseMapPointMatch) and the observation leaves the point's list (pMP->EraseObservation, C/src/MapPoint.cc:192-217: mpRefKF moves to the first
 *     remaining observation if it was that keyframe; nObs -- 2 per stereo, 1 per monocular observation, an observation whose keyframe is outside the problem
 *     counts 1, one in a CORB_KF_BAD keyframe of the problem keeps its weight (it has no edge) -- <= 2 => SetBadFlag (:255-269): CORB_MP_BAD, n_obs = 0, the matches in its remaining keyframes OF THE PROBLEM cleared)
 *   Tcw of the local keyframes that are not CORB_KF_FIXED; world_pos of the local points that are not CORB_MP_FIXED, followed by
 *     MapPoint::UpdateNormalAndDepth (:424-472) over the observations whose keyframes are in the problem (the reference's window holds every observer:
 *     :530-545), with mvScaleFactors rebuilt from scale_factor (= ORBextractor's scaleFactor, 1.2 in every reference yaml) as ORBextractor.cc:418-424 does.
 * result->poses (n_kf x 16) / points (n_mp x 3): optional copies of the estimates.  erase_pairs[k] = (index into kf_slots, index into mp_slots) of the
 * k-th outlier observation in edge order (points in mp_slots order, within a point mObservations order); *n_erase = their number (may exceed erase_cap:
 * only the first erase_cap are stored). */
int corb_local_ba_store(CorbKfStore* kf, const int32_t* kf_slots, int n_local, int n_kf, CorbMpStore* mp, const int32_t* mp_slots, int n_mp,
                        const CorbBAStage* stages, int n_stages, float scale_factor, int apply_erase, volatile int* stop_flag,
                        CorbBAResult* result, int32_t* erase_pairs, int erase_cap, int* n_erase, const CorbBAOptions* options);

/* ---- tracking-thread calls on device-resident records ----
 * The current and the last Frame are records of a keyframe store (features, mvuRight, per-feature MapPoint ids = mvpMapPoints, pose, mvInvLevelSigma2;
 * record flag bit 1 of a feature = mvbOutlier), the map is a map-point store.  Nothing but a pose, a count and (optionally) the match array crosses PCIe.
 * corb_mp_store_build_index: mnId -> slot table (device memory, kept by the store) over slots first .. first+n; rebuild after records were added or moved.
 * CORB_ERR_ARG if two of the slots hold the same id. */
int corb_mp_store_build_index(CorbMpStore* s, int first, int n);
/* features of the record in `slot` as the host knows them (-1: empty slot, or filled from a device-side count) */
int corb_kf_store_count(CorbKfStore* s, int slot);
typedef struct CorbTrackCamera {
    float fx, fy, cx, cy, bf, mb;                 /* Frame::fx ... mbf, mb */
    float min_x, max_x, min_y, max_y;             /* mnMinX ... mnMaxY */
    int32_t nlevels; float scale[16];             /* mvScaleFactors */
} CorbTrackCamera;
/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono) (C/src/ORBmatcher.cc:1470-1614) with
 * CurrentFrame = record cur_slot, LastFrame = record last_slot of `frames`: the last frame's features that hold a non-bad MapPoint of `map` and are not
 * outliers are projected with Tcw (the current frame's predicted pose; Tlw = the last frame's pose, for the forward / backward test), matched like
 * corb_search_by_projection_frame (same kernels), and CurrentFrame.mvpMapPoints[f] = the matched MapPoint's id is written into the record.  match (optional,
 * n(cur_slot) entries) = index of the last-frame feature or -1; *n_matches = the return value. */
int corb_track_search_last_frame(CorbKfStore* frames, int cur_slot, int last_slot, CorbMpStore* map, const float* Tcw /* 16 */, const float* Tlw /* 16 */,
                                 const CorbTrackCamera* cam, float th, int mono, float nnratio, int check_orientation, int32_t* match, int* n_matches);
/* int Optimizer::PoseOptimization(Frame *pFrame) (C/src/Optimizer.cc:272-485) on record `slot`: one edge per feature whose MapPoint id resolves to a non-bad
 * record of `map` (stereo iff mvuRight >= 0, information mvInvLevelSigma2[octave] of the record), start pose Tcw_in, the four rounds of the reference in ONE
 * kernel (as corb_pose_optimization_batch); mvbOutlier goes to the record's feature flags, the pose into the record (and Tcw_out); returns nInitialCorrespondences-nBad
 * in *n_inliers.  outlier (optional, n(slot) entries) = mvbOutlier.  discard_outliers: the "Discard outliers" loop of TrackWithMotionModel / TrackReferenceKeyFrame
 * (C/src/Tracking.cc:795-814, 919-940) on the record: an outlier feature loses its MapPoint and its mvbOutlier flag, and the point counts as seen in this frame
 * (mnLastFrameSeen: corb_track_search_local_points skips it); `outlier` still reports which features were rejected.  A pose optimisation with discard_outliers = 0
 * leaves mvbOutlier set, which the next frame's corb_track_search_last_frame honours (TrackLocalMap, Tracking.cc:1063-1083 keeps them too). */
int corb_track_pose_optimization(CorbKfStore* frames, int slot, CorbMpStore* map, const CorbTrackCamera* cam, const float* Tcw_in /* 16 */, float* Tcw_out /* 16 */,
                                 int discard_outliers, uint8_t* outlier, int32_t* n_inliers);
/* void Tracking::SearchLocalPoints() (C/src/Tracking.cc:1168-1216) on record `slot` with Tcw = the frame's current pose: bad MapPoints leave the frame; the
 * local MapPoints local_ids (mvpLocalMapPoints as ids; unknown ids and bad points are skipped) that the frame does not hold yet go through
 * Frame::isInFrustum(pMP, 0.5) (C/src/Frame.cc:270-329, MapPoint::PredictScale C/src/MapPoint.cc:500-514 with log_scale_factor = mfLogScaleFactor) on the
 * device, then ORBmatcher(nnratio).SearchByProjection(Frame&, vpMapPoints, th) (ORBmatcher.cc:45-131; the kernels of corb_search_by_projection_map) and
 * F.mvpMapPoints[f] = the matched id is written into the record.  match (optional, n(slot) entries) = index into local_ids or -1; tracked (optional,
 * n_local entries) = what isInFrustum left in the MapPoints (mbTrackInView -> valid); *n_in_view = nToMatch. */
int corb_track_search_local_points(CorbKfStore* frames, int slot, CorbMpStore* map, const uint64_t* local_ids, int n_local, const CorbTrackCamera* cam,
                                   const float* Tcw /* 16 */, float log_scale_factor, float th, float nnratio, int32_t* match, CorbTrackedPoint* tracked,
                                   int* n_matches, int* n_in_view);

/* int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th) (C/src/ORBmatcher.cc:960-1116) on records -- what
 * LocalMapping::SearchInNeighbors runs per neighbour keyframe (C/src/LocalMapping.cc:475-560).  pKF = record `slot` of `kf` (features, mvuRight, descriptors;
 * Tcw = pKF->GetPose(), the camera centre is derived from it; cam = intrinsics, image bounds, mvScaleFactors, from which mvInvLevelSigma2 follows as
 * ORBextractor.cc:418-430 builds it); vpMapPoints = the records mp_slots of `map`.  A point takes part unless it is bad or already observed by pKF
 * (pMP->IsInKeyFrame(pKF), :990-993: its observation list holds the keyframe's id).  The search is corb_fuse's (same kernels, sim3 = 0):
 * best_idx[i] = the feature point i is fused into or -1, best_dist[i], *n_fused = the return value.
 * action[i] (optional): 0 not fused; 1 the feature held no MapPoint (:1097-1101) and point i is the first of vpMapPoints fused into it -- with apply != 0 the
 * records are updated as the reference does: pMP->AddObservation(pKF, bestIdx) (the observation enters the point's list in ascending keyframe id) and
 * pKF->AddMapPoint(pMP, bestIdx) (the keyframe record's map-point id of that feature); 2 the feature holds a MapPoint -- from before the call, or an earlier
 * point of this call -- i.e. the reference's MapPoint::Replace of the one with fewer observations (:1085-1096), which re-links whole observation lists:
 * left to the caller, in ascending i; 3 as 1, but the point's record has no room for another observation: nothing written, CORB_ERR_CAPACITY returned. */
int corb_fuse_store(CorbKfStore* kf, int slot, CorbMpStore* map, const int32_t* mp_slots, int n_points, const CorbTrackCamera* cam,
                    const float* Tcw /* 16 */, float log_scale_factor, float th, int apply, int32_t* best_idx, int32_t* best_dist, uint8_t* action, int* n_fused);

/* The part of MapPoint's serialised state (C/include/MapPoint.h:52-72) the 112-byte CorbMapPointRecord does not carry -- mnVisible, mnFound, mpReplaced -- lives in the 16
 * spare bytes of a record's 128-byte header on the device: zero after corb_mp_store_put, moved with the record by a push.  replaced_by: 0 = mpReplaced is NULL, else id + 1. */
typedef struct CorbMapPointCounters { int32_t n_visible, n_found; uint64_t replaced_by; } CorbMapPointCounters;
int corb_mp_store_set_counters(CorbMpStore* s, int first, int n, const CorbMapPointCounters* counters);
int corb_mp_store_get_counters(CorbMpStore* s, int first, int n, CorbMapPointCounters* counters);
/* int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint) (C/src/ORBmatcher.cc:1118-1241) on
 * records -- what SearchAndFuse runs per keyframe of CorrectedSim3 (S/src/GlobalOptimize.cpp:406-432, C/src/LoopClosing.cc:594-620).  Scw = Converter::toCvMat(g2oScw),
 * 16 floats; the rest as corb_fuse_store.  The search is corb_fuse's with sim3 = 1 (same kernels).  A point takes part unless it is bad or the keyframe RECORD holds
 * its id at some feature (spAlreadyFound = pKF->GetMapPoints(), :1131, :1143 -- not IsInKeyFrame through the observation list, as the SE3 form tests).  The map's id
 * index is needed (none: CORB_ERR_ARG).  action[i] (optional) and replace_slot[i]:
 *   0  not fused (replace_slot -1)
 *   1  the feature held no point and point i is the first of the list fused into it; with apply != 0 AddObservation and AddMapPoint happen on the records exactly as
 *      in corb_fuse_store (3: the point's observation list is full, nothing written, CORB_ERR_CAPACITY returned); a point whose list holds the keyframe already
 *      (it observes the keyframe, the record no longer holds it) keeps its list, as MapPoint::AddObservation returns at once, and enters the feature
 *   2  the feature holds a non-bad point, from before the call or from an earlier point of this call: replace_slot[i] = its slot = vpReplacePoint[i].  The caller then
 *      runs corb_mp_store_replace(map, replace_slot[i], mp_slots[i], ...) in ascending i -- pRep->Replace(mvpLoopMapPoints[i]), GlobalOptimize.cpp:423-430.  A feature
 *      whose id resolves to no record of the index is reported like this too, as corb_fuse_store reports it, with replace_slot -1: there is nothing to replace
 *   4  the feature holds a point that is bad: counted in *n_fused, nothing is done (:1227-1231)
 * The actions are decided from the record as it stands before the call, so apply == 0 reports what apply != 0 does. */
int corb_fuse_sim3_store(CorbKfStore* kf, int slot, CorbMpStore* map, const int32_t* mp_slots, int n_points, const CorbTrackCamera* cam,
                         const float* Scw /* 16 */, float log_scale_factor, float th, int apply, int32_t* best_idx, int32_t* best_dist, int32_t* replace_slot,
                         uint8_t* action, int* n_fused);
/* The tracking / local-mapping / loop-closing scratch of MapPoint's serialised state (C/include/MapPoint.h:52-72) that neither the 112-byte header nor the counters carry:
 * with it a record holds EVERY field the reference's boost archive moves, so a push is a faithful stand-in for the archive.  It lives behind the observation lists of the
 * record (corb_mp_store_record_bytes covers it), is zero after corb_mp_store_put and travels with the record in corb_map_push_ex; the kernels of this library do not read it,
 * with one exception: corb_loop_correct_store reads and writes corrected_by_kf and corrected_reference. */
typedef struct CorbMapPointScratch {
    int64_t first_kf_id, first_frame;           /* mnFirstKFid, mnFirstFrame */
    uint64_t track_reference_for_frame, last_frame_seen;      /* mnTrackReferenceForFrame, mnLastFrameSeen */
    uint64_t ba_local_for_kf, fuse_candidate_for_kf, loop_point_for_kf, corrected_by_kf, corrected_reference;      /* mnBALocalForKF ... mnCorrectedReference */
    float track_proj_x, track_proj_y, track_proj_xr, track_view_cos;      /* mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos */
    int32_t track_scale_level;                  /* mnTrackScaleLevel */
    int32_t n_obs_weight;                       /* nObs (2 per stereo observation, 1 per monocular one) */
    uint8_t track_in_view; uint8_t pad[7];      /* mbTrackInView */
} CorbMapPointScratch;                          /* 104 bytes */
int corb_mp_store_set_scratch(CorbMpStore* s, int first, int n, const CorbMapPointScratch* scratch);
int corb_mp_store_get_scratch(CorbMpStore* s, int first, int n, CorbMapPointScratch* scratch);
/* void MapPoint::Replace(MapPoint* pMP) (C/src/MapPoint.cc:277-316) on records: this = record slot_this, pMP = record slot_into of `map`; the keyframes are looked up by id among
 * the slots [kf_first, kf_first + kf_n) of `kf` (an observing keyframe that is not among them keeps its record; the observation lists are re-linked regardless).
 * As the reference: nothing if both are the same point; this loses its observations, becomes bad, mpReplaced = pMP; every observation (pKF, idx) of this, in list order, either
 * moves to pMP -- pKF->ReplaceMapPointMatch(idx, pMP) in the keyframe's record, pMP->AddObservation(pKF, idx) at its place in the ascending list -- or, when pMP is in that
 * keyframe already, is erased there (pKF->EraseMapPointMatch(idx)); pMP->IncreaseFound / IncreaseVisible by this' counters; pMP->ComputeDistinctiveDescriptors() over its
 * observations in non-bad keyframes of the named slots (same selection as corb_distinctive_descriptors).  *status: 0 done, 1 the same point.  CORB_ERR_CAPACITY (nothing
 * written) if pMP's observation list has no room.  What corb_fuse_store reports as action 2 is resolved with this call, point by point, in ascending order. */
int corb_mp_store_replace(CorbMpStore* map, int slot_this, int slot_into, CorbKfStore* kf, int kf_first, int kf_n, int* status);

/* int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist) (C/src/ORBmatcher.cc:1616-1744) on records --
 * the projection step of Tracking::Relocalization (C/src/Tracking.cc:1440-1500), which passes the MapPoints the frame holds as sAlreadyFound.  CurrentFrame = record
 * cur_slot of `frames` (Tcw = its pose estimate), pKF = record kf_slot of `kfs` (the same store or another one on the same device): pKF's features whose MapPoint id
 * resolves to a non-bad record of `map` and is not held by the frame are projected and matched like corb_search_by_projection_reloc (same kernels: closed image test,
 * octaves level-1 .. level+1, a frame feature that holds a MapPoint is skipped, rotation histogram when check_orientation); CurrentFrame.mvpMapPoints[f] = the matched id is
 * written into the frame's record.  match (optional, n(cur_slot) entries) = pKF feature index or -1; *n_matches = the return value. */
int corb_track_search_reloc(CorbKfStore* frames, int cur_slot, CorbKfStore* kfs, int kf_slot, CorbMpStore* map, const CorbTrackCamera* cam,
                            const float* Tcw /* 16 */, float log_scale_factor, float th, int orb_dist, int check_orientation, int32_t* match, int* n_matches);
/* int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th) (C/src/ORBmatcher.cc:425-538) on
 * records -- the projection search of a loop / map-fusion event right before CorrectLoop and the global BA (C/src/LoopClosing.cc:377; S/src/GlobalOptimize.cpp:199).
 * pKF = record `slot` of `kf`; vpPoints = the records mp_slots of `map` (the loop keyframe's covisible points); vpMatched = matched_ids, n(slot) MapPoint ids
 * (CORB_NO_MAP_POINT = NULL), read and written: a point takes part unless it is bad or its id is among matched_ids on entry, a feature that holds an id is skipped, and
 * matched_ids[idx] = the id of the point matched to feature idx.  Same kernels as corb_search_by_projection_scw.  match (optional, n(slot) entries) = index into
 * mp_slots or -1 (this call's matches only); *n_matches = the return value. */
int corb_search_by_projection_scw_store(CorbKfStore* kf, int slot, CorbMpStore* map, const int32_t* mp_slots, int n_points, const CorbTrackCamera* cam,
                                        const float* Scw /* 16 */, float log_scale_factor, float th, uint64_t* matched_ids, int32_t* match, int* n_matches);
/* int ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, s12, R12, t12, th) (C/src/ORBmatcher.cc:1244-1468) on records -- LoopClosing::ComputeSim3's
 * guided search (C/src/LoopClosing.cc:318-330).  pKF1 / pKF2 = records slot1 / slot2 of `kf` (T1w / T2w = their poses; cam = pKF1's intrinsics, used for both directions as
 * the reference does); vpMatches12 on entry = matched12_ids (MapPoint ids per feature of KF1, CORB_NO_MAP_POINT = none; NULL = none at all): such a feature is skipped, and
 * so is the feature of KF2 that observes the matched point (GetIndexInKeyFrame through the point's observation list).  Same kernels as corb_search_by_sim3 in both
 * directions, agreement check on the host.  match12[i1] = feature of KF2 or -1 (new matches only, as in the host-array call); match12_ids (optional) = the MapPoint id
 * that feature holds, i.e. the new vpMatches12[i1]; *n_found = the return value. */
int corb_search_by_sim3_store(CorbKfStore* kf, int slot1, int slot2, CorbMpStore* map, const CorbTrackCamera* cam, float log_scale_factor,
                              const float* T1w /* 16 */, const float* T2w /* 16 */, const uint64_t* matched12_ids, float s12, const float* R12 /* 9 */, const float* t12 /* 3 */, float th,
                              int32_t* match12, uint64_t* match12_ids, int* n_found);

/* ============================ CreateNewMapPoints (LocalMapping thread) =====================
 * The triangulation loop of LocalMapping::CreateNewMapPoints (C/src/LocalMapping.cc:262-418): what turns the pairs of SearchForTriangulation into MapPoints.
 * Per pair (:268-398): the parallax test, linear triangulation or KeyFrame::UnprojectStereo, the two depth tests, the two reprojection tests, the scale test.
 * Numerics: the reference's float expressions as non-fused IEEE operations; the stereo parallax cos(2 atan2(mb / 2, depth)) is evaluated as
 * (d^2 - h^2) / (d^2 + h^2) in double and rounded once; the null vector of the float 4x4 system A comes from a one-sided Jacobi SVD of A in FP64, rounded to float.
 * status of a pair (x3d is written whenever a point was computed, also where a later test rejects it; else 0): */
#define CORB_NP_OK           0
#define CORB_NP_NO_PARALLAX  1   /* :320-321 no stereo and very low parallax */
#define CORB_NP_W_ZERO       2   /* :310 */
#define CORB_NP_BEHIND_1     3   /* :327 */
#define CORB_NP_BEHIND_2     4   /* :331 */
#define CORB_NP_REPROJ_1     5   /* :345 / :354 */
#define CORB_NP_REPROJ_2     6   /* :368 / :377 */
#define CORB_NP_SCALE        7   /* :388, :397 */
/* source of x3d: 0 the SVD, 1 UnprojectStereo of keyframe 1, 2 UnprojectStereo of keyframe 2.  Two quirks of the reference are kept: with both sides stereo only
 * side 1's stereo parallax is evaluated (`else if`, :290), and the second keyframe's stereo reprojection uses the CURRENT keyframe's mbf (:372). */
typedef struct CorbNewPointSide {     /* one keyframe as CreateNewMapPoints reads it */
    const CorbKeyPoint* keys_un; const float* u_right; const float* depth; int32_t n;      /* mvKeysUn, mvuRight, mvDepth */
    float Tcw[16]; float fx, fy, cx, cy, bf, mb;
    const float* scale; int32_t nlevels;          /* mvScaleFactors; mvLevelSigma2 = scale^2 in float */
} CorbNewPointSide;
/* the pairs of ONE corb_search_for_triangulation call (kf1 = mpCurrentKeyFrame, kf2 = the neighbour): x3d n_pairs x 3, status / source n_pairs,
 * *n_new = pairs with CORB_NP_OK.  Host pointers; synchronous. */
int corb_triangulate_pairs(const CorbNewPointSide* kf1, const CorbNewPointSide* kf2, const int32_t* pairs, int n_pairs,
                           float* x3d /* n_pairs x 3 */, uint8_t* status, uint8_t* source, int* n_new, int device);
/* The whole neighbour loop (:219-419) on records: mpCurrentKeyFrame = record cur_slot of `kf`, vpNeighKFs = the records nb_slots (distinct, not cur_slot; the caller
 * has applied the baseline test :225-239) with F12 / epipole per neighbour as corb_search_for_triangulation_slots takes them (ComputeF12 stays with the adapter).
 * Poses and intrinsics come from the records' meta, mb and mvScaleFactors from cam.  Neighbour j is matched by the kernels of corb_search_for_triangulation_slots
 * with check_orientation = 0 (CreateNewMapPoints builds ORBmatcher(0.6, false)) against the current keyframe's has-a-map-point flags as they stand after
 * neighbours 0 .. j-1: a feature whose pair reached CORB_NP_OK is flagged from then on.  The pairs of neighbour j, ascending in idx1, are entries
 * pair_offset[j] .. pair_offset[j+1] of pairs (x 2) / x3d (x 3) / status / source; room for n_nb x n(cur_slot) entries.  *n_new = pairs with CORB_NP_OK.
 * apply == 0: no record changes (map may be NULL).  apply != 0: for the k-th OK pair in (neighbour, idx1) order record first_mp_slot + k of `map` becomes the new
 * MapPoint (:401-415): id = first_mp_id + k, ref_kf_id = the current keyframe's id, client_id, world_pos = x3d, the two observations in ascending keyframe id,
 * descriptor by the rule of corb_distinctive_descriptors (two observations: the first one's), normal / min_distance / max_distance as MapPoint::UpdateNormalAndDepth
 * computes them for the two observations, counters and scratch zero; the id and the has-a-map-point flag enter both keyframe records' features (two pairs of one
 * neighbour that share idx2 leave the later id there, as AddMapPoint does).  Fewer than *n_new records from first_mp_slot on: CORB_ERR_CAPACITY, no record written
 * (the outputs are complete).  corb_mp_store_build_index again afterwards.  One synchronisation and one read-back per call; locks as corb_fuse_store. */
int corb_create_new_map_points_store(CorbKfStore* kf, int cur_slot, const int32_t* nb_slots, int n_nb,
        const float* F12 /* n_nb x 9 */, const float* epipole /* n_nb x 2 */, const CorbTrackCamera* cam,
        int only_stereo, int apply, CorbMpStore* map, int first_mp_slot, uint64_t first_mp_id, int32_t client_id,
        int32_t* pair_offset /* n_nb + 1 */, int32_t* pairs, float* x3d, uint8_t* status, uint8_t* source, int* n_new);

/* ============================ Sim3Solver RANSAC (LoopClosing::ComputeSim3) =====================
 * C/src/Sim3Solver.cc for all candidates of a loop / map-fusion event in one call: up to max_iterations hypotheses per candidate, one wavefront each -- the three
 * draws (:163-177), ComputeSim3 (Horn on 3 points, :226-337), CheckInliers (:340-364) -- and iterate()'s stateful loop (:158-201) as a rule over the per-hypothesis
 * inlier counts c_i: iteration i returns (an *event*) iff c_i > min_inliers and c_i >= max_{j<i} c_j.  The reference seeds rand() from the clock, so the draws are an
 * input: rand_values = n x max_iterations x 3 results of rand() in [0, 2^31) (RAND_MAX + 1 = 2^31), consumed as DUtils::Random::RandomInt does
 * (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) with the swap-with-back removal of :175-176.
 * Numerics: the reference's expressions as non-fused IEEE operations with the C++ types of the source; cv::eigen of the float 4x4 N = a cyclic
 * Jacobi iteration on N in FP64 (column of the largest diagonal entry, rounded to float); atan2 + cv::Rodrigues = R = I + (2 q0 [v]x + 2 [v]x^2) / |q|^2 in double,
 * each entry rounded once.  A hypothesis whose quaternion has a zero vector part (the reference divides 0 by 0, :280) or any non-finite R, t, s has no inliers. */
typedef struct CorbSim3RansacProblem {          /* what the constructor (:37-112) leaves, flattened by the adapter */
    int32_t n;                                  /* N = mvpMapPoints1.size() */
    const float* p1c; const float* p2c;         /* n x 3: mvX3Dc1, mvX3Dc2 (:94-98) */
    const float* sigma2_1; const float* sigma2_2;      /* n: mvLevelSigma2[kp.octave] of both sides (:84-85); the library applies 9.210 * sigma2, truncated (:87-88) */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;      /* mK1, mK2 (:105-106) */
} CorbSim3RansacProblem;
typedef struct CorbSim3RansacEvent {            /* one return of iterate() with a transformation (:192-199) */
    int32_t iteration;                          /* mnIterations at the return, 1-based */
    int32_t n_inliers;                          /* nInliers */
    float R12[9], t12[3], s12;                  /* mBestRotation, mBestTranslation, mBestScale; T12 = [s12 R12 | t12] */
} CorbSim3RansacEvent;
/* SetRansacParameters(probability, min_inliers, max_iterations) (:114-138) + every iterate() a caller could make, per problem: ransac_max_its = mRansacMaxIts (0 with no
 * events when n < min_inliers: bNoMore at once, :146-150); n_events = all events (may exceed max_events); events / inlier_flags = the first max_events of them, flags one
 * byte per correspondence (mvbInliersi) in rows of flags_stride >= every n.  counts (optional, n_problems x max_iterations) = c_i, q_out (optional, x 4) = the
 * quaternion of hypothesis i; entries from ransac_max_its on are 0.  min_inliers < 3, probability outside (0, 1), max_iterations outside [1, 65535] or a rand_values
 * entry outside [0, 2^31): CORB_ERR_ARG, nothing written.  Host pointers; one synchronisation and one read-back per call. */
int corb_sim3_ransac(const CorbSim3RansacProblem* problems, int n_problems, double probability, int min_inliers, int max_iterations, int fix_scale,
                     const int32_t* rand_values /* n_problems x max_iterations x 3 */, int max_events, int flags_stride,
                     int32_t* ransac_max_its /* n_problems */, int32_t* n_events /* n_problems */, CorbSim3RansacEvent* events /* n_problems x max_events */,
                     uint8_t* inlier_flags /* n_problems x max_events x flags_stride */, int32_t* counts, float* q_out, int device);
/* The same on records, constructor included (:37-112): pKF1 = record slot1 of `kf`, candidate c = record slots2[c] (not slot1), vpMatched12 of candidate c =
 * matched12_ids[c x n(slot1) ..] as MapPoint ids (CORB_NO_MAP_POINT = NULL) -- what corb_search_by_bow_slots + the records' map-point ids give.  Feature i1 is kept when
 * KF1 holds a MapPoint there, both ids resolve through the map's index (corb_mp_store_build_index) to records that are not bad, and GetIndexInKeyFrame finds both
 * keyframes in the points' observation lists (:64-79); the keypoints are those at the observation indices (:81-82).  Poses and intrinsics come from the records' meta,
 * sigma2 = scale[octave]^2 in float from cam1 / cam2[c] as CorbNewPointSide reads it.  n_corr[c] = N, index1 (optional, n_candidates x n(slot1)) = mvnIndices1 (-1 behind
 * N); inlier_flags rows have n(slot1) bytes and are scattered through mvnIndices1: the vbInliers of iterate() (:195-197).  No record changes.  Locks as corb_fuse_store. */
int corb_sim3_ransac_store(CorbKfStore* kf, int slot1, const int32_t* slots2, int n_candidates, CorbMpStore* map, const CorbTrackCamera* cam1,
                           const CorbTrackCamera* cam2 /* n_candidates */, const uint64_t* matched12_ids /* n_candidates x n(slot1) */,
                           double probability, int min_inliers, int max_iterations, int fix_scale, const int32_t* rand_values, int max_events,
                           int32_t* ransac_max_its, int32_t* n_events, CorbSim3RansacEvent* events, uint8_t* inlier_flags /* n_candidates x max_events x n(slot1) */,
                           int32_t* n_corr /* n_candidates */, int32_t* index1, int32_t* counts, float* q_out);

/* ============================ PnPsolver RANSAC (Tracking::Relocalization, MapFusion) ============
 * C/src/PnPsolver.cc for all candidates of a relocalisation / map-fusion step in one call: per candidate mRansacMaxIts + tail_iterations hypotheses, one wavefront each
 * -- the min_set draws (:233-246), EPnP's compute_pose (:522-570) and CheckInliers (:353-384) -- then Refine() (:305-350) for every hypothesis that changes the running
 * best, and iterate()'s state (:210-303) as a rule over the per-hypothesis inlier counts c_i, with m = mRansacMinInliers after SetRansacParameters' adjustment:
 * iteration i is a *record* iff c_i >= m and c_i > every earlier c_j >= m; b(i) = the last record at or before i; Refine() depends only on the record and is ok iff its
 * own count is > m; iteration i returns the refined pose of b(i) iff c_i >= m and b(i) is ok (a later non-record i returns the same pose again).  The loop condition of
 * :227 is an OR: a call from mnIterations = s runs to an event or to max(mRansacMaxIts, s + nIterations), where it sets bNoMore and returns the last record's unrefined
 * pose if there is one (:286-300) -- hence tail_iterations, the hypotheses evaluated behind the cap.  corb::pnp_replay (host/corb_host.hpp) states that rule.
 * The reference seeds rand() from the clock, so the draws are an input: rand_values = per problem (max_iterations + tail_iterations) x min_set results of rand() in
 * [0, 2^31), consumed as DUtils::Random::RandomInt does, with the swap-with-back removal of :244-245.
 * Numerics (csrc/pnp_math.h is the text, tests/pnpsolver_reference.py the definition): the source's double expressions, unfused, sums over
 * correspondences in ascending order; cvSVD of the symmetric PW0tPW0 and MtM = a cyclic Jacobi eigen-iteration in FP64; cvInvert / cvSolve(CV_SVD) / cvSVD(ABt) = a
 * one-sided Jacobi SVD in FP64 whose terms with w_k <= 2 DBL_EPSILON sum_j w_j are dropped.  NaN and infinity flow through as in the source: such a hypothesis has no
 * inliers because error2 < mvMaxError is false. */
typedef struct CorbPnPRansacProblem {           /* what the constructor (:67-110) leaves */
    int32_t n;                                  /* N = mvP2D.size() */
    const float* p3dw;                          /* n x 3: mvP3Dw */
    const float* p2d;                           /* n x 2: mvP2D (mvKeysUn[i].pt) */
    const float* sigma2;                        /* n: mvSigma2; the library applies mvMaxError = sigma2 * th2 (:199-201) */
    float fx, fy, cx, cy;                       /* fu, fv, uc, vc (:104-107) */
} CorbPnPRansacProblem;
typedef struct CorbPnPRansacRecord {            /* one change of the running best (:257-269) and its Refine() (:305-350) */
    int32_t iteration;                          /* mnIterations at the change, 1-based */
    int32_t n_inliers;                          /* mnBestInliers */
    float Tcw_best[12];                         /* rows 0-2 of mBestTcw: the convertTo(CV_32F) of :262-268 */
    int32_t n_refined;                          /* mnRefinedInliers */
    int32_t refine_ok;                          /* Refine()'s return: n_refined > mRansacMinInliers */
    float Tcw_refined[12];                      /* rows 0-2 of mRefinedTcw (written whatever refine_ok is) */
} CorbPnPRansacRecord;
/* SetRansacParameters(probability, min_inliers, max_iterations, min_set, epsilon, th2) (:166-202) + everything iterate() could return, per problem: ransac_max_its =
 * mRansacMaxIts (0 with no records when n < ransac_min_inliers: bNoMore at once, :218-222), ransac_min_inliers = the adjusted mRansacMinInliers; hypotheses
 * 0 .. ransac_max_its + tail_iterations - 1 are evaluated.  n_records = all records (may exceed max_records); records / best_flags / refined_flags = the first
 * max_records of them, flags one byte per correspondence (mvbBestInliers, mvbRefinedInliers) in rows of flags_stride >= every n.  counts (optional, n_problems x
 * (max_iterations + tail_iterations)) = c_i; pose_out (optional, x 16 doubles) = R[9], t[3], rep_errors[1..3] and the chosen N of hypothesis i; refine_pose_out
 * (optional, n_problems x max_records x 16) = the same of each record's Refine(); entries behind the evaluated hypotheses / records are 0.  min_set outside 4..8,
 * min_inliers < min_set, probability outside (0, 1), epsilon outside (0, 1], max_iterations outside [1, 65535], tail_iterations outside [0, 65535] or a rand_values entry
 * outside [0, 2^31): CORB_ERR_ARG, nothing written.  Host pointers; three launches, one synchronisation and one read-back per call. */
int corb_pnp_ransac(const CorbPnPRansacProblem* problems, int n_problems, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                    int tail_iterations, const int32_t* rand_values /* n_problems x (max_iterations + tail_iterations) x min_set */, int max_records, int flags_stride,
                    int32_t* ransac_max_its /* n_problems */, int32_t* ransac_min_inliers /* n_problems */, int32_t* n_records /* n_problems */,
                    CorbPnPRansacRecord* records /* n_problems x max_records */, uint8_t* best_flags /* n_problems x max_records x flags_stride */,
                    uint8_t* refined_flags /* the same */, int32_t* counts, double* pose_out, double* refine_pose_out, int device);
/* The same on records, constructor included (:67-110 over a Frame, :112-155 over a KeyFrame): the frame = record `slot` of `frames`, one candidate per row of
 * vvpMapPointMatches: matched_ids[c x n(slot) ..] as MapPoint ids (CORB_NO_MAP_POINT = NULL) -- what corb_search_by_bow_slots + the candidate records' map-point ids give.
 * Feature i is kept when its id resolves through the map's index (corb_mp_store_build_index) to a record that is not bad; mvP2D = mvKeysUn[i].pt of the frame record,
 * mvSigma2 = scale[octave]^2 in float from cam, mvP3Dw = the map-point record's world position, fu, fv, uc, vc = the frame record's meta.  n_corr[c] = N, index (optional,
 * n_candidates x n(slot)) = mvKeyPointIndices (-1 behind N); both flag sets have rows of n(slot) bytes and are scattered through mvKeyPointIndices: the vbInliers of
 * iterate() (:274-279, :292-297).  Five launches (prepare, scan, compaction, hypotheses, Refine).  No record changes.  Locks as corb_sim3_ransac_store. */
int corb_pnp_ransac_store(CorbKfStore* frames, int slot, CorbMpStore* map, const CorbTrackCamera* cam, const uint64_t* matched_ids /* n_candidates x n(slot) */,
                          int n_candidates, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2, int tail_iterations,
                          const int32_t* rand_values, int max_records, int32_t* ransac_max_its, int32_t* ransac_min_inliers, int32_t* n_records,
                          CorbPnPRansacRecord* records, uint8_t* best_flags /* n_candidates x max_records x n(slot) */, uint8_t* refined_flags,
                          int32_t* n_corr /* n_candidates */, int32_t* index, int32_t* counts, double* pose_out, double* refine_pose_out);

/* ============================ Initializer (Tracking::MonocularInitialization) ============
 * C/src/Initializer.cc for the (reference, current) frame pairs of several clients in one call: Initialize (:44-121) -- the 8-point sets of every iteration (:77-97),
 * FindHomography (:124-172) and FindFundamental (:175-223) as 2 x max_iterations independent hypotheses per problem, one wavefront each, over the same sets -- then RH
 * and the model (:112-118), the 4 motion hypotheses of DecomposeE (:909-929) or the 8 of :584-686, a CheckRT (:798-907) per hypothesis, and the decision of ReconstructF
 * (:499-569) or ReconstructH (:689-731).  Tracking.cc:620 calls it once per frame until it succeeds.
 * DUtils::Random::SeedRandOnce(0) seeds only the first call of a process and the stream is shared with every other RANSAC, so the draws are an input: rand_values = per
 * problem max_iterations x 8 results of rand() in [0, 2^31), each consumed as RandomInt(0, size - 1) with the swap-with-back removal of :94-95; H and F share the sets.
 * Numerics (csrc/init_math.h is the text, tests/initializer_reference.py the definition): the source's float expressions, unfused, in the types C++
 * gives them; Normalize (:749-795) over all keys of a frame and the scores (:363, :379, :441, :459) are float sums in ascending index order -- the score decides which
 * hypothesis wins, so its order is part of the definition; cv::SVDecomp / cv::SVD::compute = a one-sided Jacobi SVD in FP64 rounded to float once (the sign of a null
 * vector is whatever the iteration leaves: H is homogeneous, F enters squared, s = det U det Vt and the +-t of DecomposeE absorb it); Mat::inv() of a 3 x 3 = adjugate
 * times 1 / det in double; float products accumulate in double.  The parallax tests (:525 >, :721 >=) are made on the cosine against thresholds the host finds with its
 * own acos; the reported parallax is float(acos((double)c) * 180 / pi) of the returned cosine.  vCosParallax[min(50, size - 1)] is the order statistic by (value,
 * position), a NaN last.  Where the reference would crash -- an empty H21 / F21, RH = NaN -- the call reports a status. */
typedef struct CorbInitProblem {
    const CorbKeyPoint* keys1; int32_t n1;      /* mvKeys1 = ReferenceFrame.mvKeysUn (x, y read) */
    const CorbKeyPoint* keys2; int32_t n2;      /* CurrentFrame.mvKeysUn */
    const int32_t* matches12;                   /* n1: vMatches12, -1 = none */
    float fx, fy, cx, cy;                       /* mK */
} CorbInitProblem;
#define CORB_INIT_OK           0                /* Initialize returned true */
#define CORB_INIT_NO_MODEL     1                /* no positive finite score for the model the ratio selects, or RH is NaN */
#define CORB_INIT_H_DEGENERATE 2                /* :597: d1 / d2 or d2 / d3 below 1.00001 */
#define CORB_INIT_AMBIGUOUS    3                /* :517 nsimilar > 1, or :721 secondBestGood >= 0.75 bestGood */
#define CORB_INIT_FEW_POINTS   4                /* :517 maxGood < nMinGood, or :721 bestGood <= minTriangulated or <= 0.9 N */
#define CORB_INIT_LOW_PARALLAX 5                /* :525-565 parallax <= minParallax, or :721 bestParallax < minParallax */
typedef struct CorbInitResult {
    int32_t status;                             /* CORB_INIT_*.  Several failing tests at once: F in the order of :517-525 (few points, ambiguous, parallax), H of :721 as
                                                   parallax, ambiguous, few points */
    int32_t model;                              /* 0 = H (RH > 0.40), 1 = F */
    int32_t n_matches;                          /* N = mvMatches12.size() */
    float score_h, score_f, rh;                 /* SH, SF (0 if no hypothesis scored above 0), RH = SH / (SH + SF) */
    int32_t best_it_h, best_it_f;               /* the iteration that won, 0-based: the first maximum (the source's strict >); -1 if none */
    float H21[9], F21[9];                       /* row-major; zero if none */
    int32_t n_inliers;                          /* N of :473-476 / :575-578: the inliers of the chosen model */
    int32_t n_good[8];                          /* nGood of CheckRT per motion hypothesis in the source's order: F (R1,t) (R2,t) (R1,-t) (R2,-t); entries 4..7 unused for F */
    float cos_parallax[8];                      /* vCosParallax[min(50, size - 1)] after the sort; 1 where nGood = 0 (parallax 0, :904) */
    float parallax[8];                          /* :901, computed on the host from cos_parallax */
    int32_t best_hypothesis;                    /* F: the first hypothesis that equals maxGood (the else-if chain of :523-567 tries no other); H: bestSolutionIdx (-1 if every nGood is 0) */
    int32_t second_best_good;                   /* H: secondBestGood; F: the same rule over its four */
    float R21[9], t21[3];                       /* zero unless status = CORB_INIT_OK */
    int32_t n_triangulated;                     /* number of set entries of vbTriangulated */
} CorbInitResult;
/* Initializer(ReferenceFrame, sigma, max_iterations).Initialize(...) with ReconstructH / ReconstructF's minParallax and minTriangulated (1.0 and 50 at :116-118), per
 * problem.  rand_values: n_problems x max_iterations x 8.  p3d (n_problems x p3d_stride x 3) = vP3D and triangulated (n_problems x p3d_stride) = vbTriangulated, both by
 * key-1 index, p3d_stride >= every n1; vP3D is written even where cosParallax >= 0.99998 leaves vbTriangulated false (:889-893).  inliers_h / inliers_f (optional,
 * n_problems x flags_stride bytes, flags_stride >= every N) = vbMatchesInliersH / F, one byte per entry of mvMatches12.  scores (optional, n_problems x max_iterations x
 * 2) = currentScore of every H and F hypothesis.  On a failed status the diagnostics (scores, H21, F21, inliers, n_good, cos_parallax) stay filled and R21, t21, p3d and
 * triangulated are zero.  N < 8 (the source indexes an empty vector; Tracking never calls it below 100), a match index outside [-1, n2), max_iterations outside
 * [1, 65535], sigma <= 0 or a rand_values entry outside [0, 2^31): CORB_ERR_ARG, nothing written.  Host pointers; four launches, one synchronisation and one read-back
 * per call.  (A form on records is not built: SearchForInitialization has no slots form to chain it to.) */
int corb_mono_initialize(const CorbInitProblem* problems, int n_problems, float sigma, int max_iterations, float min_parallax, int min_triangulated,
                         const int32_t* rand_values /* n_problems x max_iterations x 8 */, int p3d_stride, int flags_stride, CorbInitResult* results /* n_problems */,
                         float* p3d, uint8_t* triangulated, uint8_t* inliers_h, uint8_t* inliers_f, float* scores, int device);

/* ============================ place recognition: DBoW2 vocabulary transform and keyframe database =============================
 * Frame::ComputeBoW / KeyFrame::ComputeBoW (C/src/Frame.cc:397-406) and C/src/KeyFrameDatabase.cc on the device.  The arithmetic is csrc/bow_math.h, the definition
 * tests/dbow_reference.py (DESIGN.md section 2 lists the readings); BowVector values, scores and the six per-keyframe fields are bit-equal to it.  Only L1_NORM scoring
 * (0) with TF_IDF weighting (0) exists -- what ORB-SLAM's vocabulary carries; anything else is CORB_ERR_ARG. */
typedef struct CorbVoc CorbVoc;
typedef struct CorbVocDesc {
    int32_t k, L, scoring, weighting;           /* the first line of the text format; k <= 20, 1 <= L <= 10 (the loader's bounds, TemplatedVocabulary.h:1359) */
    int32_t n_nodes;                            /* nodes below the root: ids 1 .. n_nodes in array order (the root is node 0) */
    const int32_t* parent;                      /* [n_nodes] id of the parent, smaller than the node's own */
    const int32_t* is_leaf;                     /* [n_nodes] > 0: a word; word ids are given in array order of the leaves */
    const uint8_t* descriptor;                  /* [n_nodes][32] */
    const double* weight;                       /* [n_nodes] read for the leaves */
} CorbVocDesc;
/* TemplatedVocabulary from flat arrays, or from the text format of loadFromTextFile (TemplatedVocabulary.h:1338-1424: `k L scoring weighting`, then one line
 * `parent isLeaf d0 .. d31 weight` per node; children keep line order; blank lines make no node).  A parent at or after its child, a leaf with children, a node that is
 * neither leaf nor parent, more than k children, k > 20 or an unsupported scoring / weighting: CORB_ERR_ARG with a message. */
int corb_voc_create(const CorbVocDesc* desc, int device, CorbVoc** out);
int corb_voc_load_text(const char* path, int device, CorbVoc** out);
void corb_voc_destroy(CorbVoc* v);
int corb_voc_info(const CorbVoc* v, int32_t* k, int32_t* L, int32_t* n_nodes /* with the root, like m_nodes.size() */, int32_t* n_words);
#define CORB_BOW_MAX_FEATURES 8192              /* features per descriptor set: one set is sorted in the LDS of one workgroup */
/* TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) (TemplatedVocabulary.h:1127-1194, :1218-1259; BowVector.cpp:34-84; FeatureVector.cpp:31)
 * for n_sets descriptor sets in one call: set s is desc[offset[s] .. offset[s + 1]) x 32 bytes, at most CORB_BOW_MAX_FEATURES features, at most 65535 sets per call.  Outputs of set s start at
 * offset[s]: bow_word / bow_value (ascending words, L1-normalised) with bow_count[s] entries; fv_node_id and fv_idx in CorbFeatVec form with fv_n_nodes[s] nodes, their
 * offsets at fv_offset[offset[s] + s ..] (n_nodes + 1 entries; the array has offset[n_sets] + n_sets entries).  feat_word / feat_node (optional, per feature) are the
 * descent's word and recorded node, stopped words included.  The node recorded is the one at depth L - levelsup, the root if that is <= 0, and the leaf itself if the
 * descent ends above that depth.  Host pointers; two launches, one synchronisation, one read-back. */
int corb_voc_transform(CorbVoc* v, const uint8_t* desc, const int32_t* offset, int n_sets, int levelsup, uint32_t* bow_word, double* bow_value, int32_t* bow_count,
                       uint32_t* fv_node_id, int32_t* fv_offset, uint32_t* fv_idx, int32_t* fv_n_nodes, int32_t* feat_word, uint32_t* feat_node);

/* KeyFrameDatabase (C/src/KeyFrameDatabase.cc:38-401) over entries 0 .. capacity_entries - 1.  An entry holds a BowVector of up to max_words words, the six fields the
 * detect functions keep per keyframe, and its GetBestCovisibilityKeyFrames(10).  These live in this object, not in the keyframe record.  The inverted file is not kept:
 * an entry's place in lKFsSharingWords is (its first word in common with the query, the sequence number of its add), which is the order the walk over
 * mvInvertedFile[word] meets it in. */
typedef struct CorbKfDb CorbKfDb;
typedef struct CorbKfDbState {                  /* mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore; all 0 for a new keyframe */
    uint64_t loop_query; int32_t loop_words; float loop_score; uint64_t reloc_query; int32_t reloc_words; float reloc_score;
} CorbKfDbState;
/* The database keeps a pointer to its vocabulary: destroy the databases of a vocabulary before the vocabulary. */
int corb_kfdb_create(CorbVoc* voc, int capacity_entries, int max_words, CorbKfDb** out);
void corb_kfdb_destroy(CorbKfDb* db);
/* mBowVec of an entry (ascending words below the vocabulary's size, every value above 0 -- what the transform produces; a value that is not is CORB_ERR_ARG, because
 * the kernels mark a word's presence in the query by its value).  Setting it makes the entry a new keyframe: its six fields are zeroed.  A live entry: CORB_ERR_ARG. */
int corb_kfdb_set_bow(CorbKfDb* db, int entry, const uint32_t* word, const double* value, int n);
int corb_kfdb_get_bow(CorbKfDb* db, int entry, uint32_t* word, double* value, int cap, int* n);
/* add (:38-46), erase (:48-65), clear (:67-70; the per-keyframe fields stay).  Adding a live entry or one without a BowVector, erasing one that is not live: CORB_ERR_ARG. */
int corb_kfdb_add(CorbKfDb* db, int entry);
int corb_kfdb_erase(CorbKfDb* db, int entry);
int corb_kfdb_clear(CorbKfDb* db);
/* GetBestCovisibilityKeyFrames(10) of n entries as entry indices in that order, -1 padded: nb[n][10] */
int corb_kfdb_set_neighbours(CorbKfDb* db, const int32_t* entries, int n, const int32_t* nb);
int corb_kfdb_get_state(CorbKfDb* db, int first_entry, int n, CorbKfDbState* out);
/* mpVoc->score(entry_a, entries_b[i]) (ScoringObject.cpp:23-68): the minScore loop of LoopClosing::DetectLoop (C/src/LoopClosing.cc:122-137) */
int corb_kfdb_score(CorbKfDb* db, int entry_a, const int32_t* entries_b, int n, double* score);
/* kind 0: DetectLoopCandidates (:73-187), 1: DetectRelocalizationCandidates (:297-401), 2: DetectMapFusionCandidatesFromDB (:189-295).  The query is any entry with a
 * BowVector, live or not (a caller keeps one entry as the current Frame's); query_id is its mnId.  connected (GetConnectedKeyFrames as entries) and min_score are read
 * for kind 0 only.  out = the candidates as entries in the reference's order, *n their number; more than cap: CORB_ERR_OVERFLOW with *n the size needed (the fields are
 * updated all the same).  One call, one synchronisation, one read-back. */
int corb_kfdb_detect(CorbKfDb* db, int kind, int query_entry, uint64_t query_id, const int32_t* connected, int n_connected, float min_score, int32_t* out, int cap, int* n);
/* Frame::ComputeBoW / KeyFrame::ComputeBoW on records: the transform of the slots' descriptors, without a host trip of descriptors or vectors.  Writes each slot's
 * FeatureVector into the record fields corb_kf_store_set_bow writes (and the host mirror of its node ids, from one small read-back), so every slots matcher works
 * unchanged, and its BowVector into entries[i] of db as corb_kfdb_set_bow would (db may be NULL: the BowVector is dropped).  The store must hold at most
 * CORB_BOW_MAX_FEATURES features per keyframe (CORB_ERR_ARG otherwise); a BowVector of more than the database's max_words words: CORB_ERR_CAPACITY, that entry is
 * left without a BowVector. */
int corb_kf_store_compute_bow(CorbKfStore* s, const int32_t* slots, int n_slots, CorbVoc* voc, int levelsup, CorbKfDb* db, const int32_t* entries);
/* Event timing of this section's launches, process-wide (corb_orb_profile's form): per kernel the summed duration and the launch count since the last read, and four
 * counters of the in-order sums taken with the device's wall clock inside the kernels -- "build: norm sum, one lane" beside "build: lane 0 in all" (bow_build_kernel), and
 * "score: ordered sum, waves" beside "score: waves in all" (kfdb_score_kernel, summed over its wavefronts); for these `launches` holds the raw ticks.  Off by default. */
int corb_bow_profile(int enable, int device);
int corb_bow_profile_read(CorbKernelTime* out, int cap, int* n);   /* resets the accumulators */

/* ============================ covisibility graph on the stores ==============================
 * KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles / EraseConnection (C/src/KeyFrame.cc:133-168, :404-502, :685-698), the covisibility queries
 * (:199-269), LocalMapping::KeyFrameCulling (C/src/LocalMapping.cc:590-648) and the window selection of Optimizer::LocalBundleAdjustment (C/src/Optimizer.cc:493-544),
 * computed on the device from the records of a keyframe store and a map-point store.  The graph object holds, per slot of `kf`, mConnectedKeyFrameWeights (every
 * counted id with its weight) and mvpOrderedConnectedKeyFrames / mvOrderedWeights (C/include/KeyFrame.h:291-293) in device memory; nothing is written into the records.
 * What the reference's words mean here:
 *   "in the cache" (Cache::KeyFrameInCache)  the id is the mnId of a slot of `kf` that holds features (of two such slots with one id: the lower); looked up per call
 *   a non-bad MapPoint                       the id resolves through the map-point store's index (corb_mp_store_build_index; none: CORB_ERR_ARG) to a record without CORB_MP_BAD
 *   MapPoint::Observations()                 derived from the observation list by corb_local_ba_store's rule: 2 for an observation whose keyframe is held and has
 *                                            u_right[idx] >= 0, else 1 (the scratch field is not read)
 * Every output is integer work and does not depend on the order the device's atomics land in.  max_connections (<= 0: 512; at most 1024) bounds the distinct ids of a
 * row: a row is sorted in the local memory of one workgroup.  Locks: the graph, then the stores as corb_fuse_store does. */
typedef struct CorbCovis CorbCovis;
int corb_covis_create(CorbKfStore* kf, CorbMpStore* mp, int max_connections, CorbCovis** out);   /* the stores outlive the graph */
void corb_covis_destroy(CorbCovis* g);
/* KeyFrame::UpdateConnections (KeyFrame.cc:404-502) for slots[0 .. n) (distinct), AS IF called one after the other in list order, AddConnection (:133-148) on the rows of
 * the listed keyframes included: the unchanged-weight early return leaves such a row's ordered list as it was, any other AddConnection rebuilds it from the row's WHOLE
 * weight map (UpdateBestCovisibles, :150-168).  th = 15 in the reference (:445).  A keyframe whose counter is empty changes nothing (:438-439).  A counter without a
 * single held keyframe (the reference dereferences NULL at :468) replaces the weight map and leaves the ordered list empty.
 * first_parent[i] (optional) = id of the front of keyframe i's ordered list after its own update -- mpParent of :493-495 if this is its first connection and its id
 * is not 0 -- or CORB_NO_MAP_POINT ("none") when there is none.  The spanning tree is kept in the graph and maintained by this call (see the tree section below).
 * CORB_ERR_CAPACITY: a counter holds more than max_connections distinct ids; detected before anything is committed, the graph is unchanged.
 * CORB_ERR_OVERFLOW: an AddConnection met a full row of ANOTHER keyframe (or the first connection's AddChild a full child set); that entry is missing, the rest of
 * the batch is applied. */
int corb_covis_update(CorbCovis* g, const int32_t* slots, int n, int th, uint64_t* first_parent);
/* the connection part of KeyFrame::SetBadFlag (KeyFrame.cc:592-595, :604-605): EraseConnection(this) (:685-698) on every keyframe of the row that the store holds, then the row cleared */
int corb_covis_erase(CorbCovis* g, int slot);
/* row -> host: the weight map in descending (weight, id) and the ordered list as it stands; more than cap entries in either: CORB_ERR_CAPACITY with the counts set */
int corb_covis_get(CorbCovis* g, int slot, uint64_t* all_id, int32_t* all_w, int* n_all, uint64_t* ord_id, int32_t* ord_w, int* n_ord, int cap);
/* GetVectorCovisibleKeyFrames (:199-211; N <= 0, min_weight <= 0), GetBestCovisibilityKeyFrames(N) (:213-230; min_weight <= 0) and GetCovisiblesByWeight(w) (:232-260;
 * min_weight = w > 0, N <= 0) as SLOTS of kf, directly usable as nb_slots / kf_slots / corb_kfdb_set_neighbours input.  The first two drop the ids the store does not hold;
 * the third keeps them as -1 and, like the reference's upper_bound followed by `it == end()`, answers an EMPTY list when every weight of the list reaches w.
 * out_w (optional) = the weights.  More than cap: CORB_ERR_CAPACITY with *n the size needed. */
int corb_covis_query(CorbCovis* g, int slot, int N, int min_weight, int32_t* out_slots, int32_t* out_w, int cap, int* n);
int corb_covis_weight(CorbCovis* g, int slot_a, int slot_b, int* w);    /* GetWeight (:262-269): weight of keyframe slot_b in the map of slot_a, 0 if none */
/* LocalMapping::KeyFrameCulling (LocalMapping.cc:590-648) for mpCurrentKeyFrame = cur_slot: per covisible keyframe, in GetVectorCovisibleKeyFrames order, its slot, nMPs,
 * nRedundantObservations and the decision `nRedundantObservations > 0.9 * nMPs` (a keyframe with mnId 0 is skipped: 0, 0, 0).  th_depth = mThDepth, read unless monocular.
 * An observation counts towards the three of :630-633 when its keyframe is held, is not this one and its feature index is below that keyframe's feature count.
 * Nothing is written: SetBadFlag stays with the caller, who then calls corb_covis_erase. */
int corb_covis_keyframe_culling(CorbCovis* g, int cur_slot, int monocular, float th_depth, int32_t* kf_slots, int32_t* n_mps, int32_t* n_redundant, uint8_t* cull, int cap, int* n);
/* the window of Optimizer::LocalBundleAdjustment (Optimizer.cc:493-544): kf_slots[0 .. n_local) lLocalKeyFrames, [n_local .. n_kf) lFixedCameras, mp_slots lLocalMapPoints,
 * in the reference's list orders (observations in ascending keyframe id) -- exactly the arguments corb_local_ba_store takes.  mnBALocalForKF / mnBAFixedForKF are
 * per-call marks; no record changes.  A window larger than kf_cap / mp_cap: CORB_ERR_CAPACITY, nothing written. */
int corb_covis_local_window(CorbCovis* g, int slot, int32_t* kf_slots, int kf_cap, int* n_local, int* n_kf, int32_t* mp_slots, int mp_cap, int* n_mp);

/* ---- the spanning tree (mpParent, mbFirstConnection, mspChildrens of C/include/KeyFrame.h) per slot of the graph's keyframe store, in device memory beside the rows ----
 * mpParent is an id or CORB_NO_MAP_POINT ("none"); a fresh graph holds none / first connection / no children for every slot.  mspChildrens is a set of ids kept in
 * ascending id (LightKeyFrame::operator<), stored explicitly and NOT derived from the parent pointers: ChangeParent never removes the keyframe from its old parent's set,
 * as in the reference.  A set holds at most max_connections ids; an insertion into a full set is skipped and answers CORB_ERR_OVERFLOW, as a full row does.
 * corb_covis_update maintains the tree as KeyFrame.cc:493-499 does, per member in list order: a member with mbFirstConnection and mnId != 0 takes the front of its ordered
 * list (after its own update) as mpParent; if the store holds that keyframe it gains the member as a child and mbFirstConnection clears.  An empty ordered list (empty
 * counter, or the no-held-keyframe reading) changes nothing. */
int corb_covis_set_tree(CorbCovis* g, int slot, uint64_t parent_id, int first_connection, const uint64_t* children, int n);   /* what an archive or a push delivers; children distinct, any order */
int corb_covis_get_tree(CorbCovis* g, int slot, uint64_t* parent_id, int* first_connection, uint64_t* children, int cap, int* n);   /* children ascending; more than cap: CORB_ERR_CAPACITY with *n set */
int corb_covis_add_child(CorbCovis* g, int slot, int child_slot);      /* KeyFrame::AddChild (KeyFrame.cc:504-508): mspChildrens.insert(child's mnId) */
int corb_covis_erase_child(CorbCovis* g, int slot, int child_slot);    /* KeyFrame::EraseChild (:510-514) */
int corb_covis_change_parent(CorbCovis* g, int slot, int other_slot);  /* KeyFrame::ChangeParent (:516-521): mpParent = other; other->AddChild(this) -- nothing else */
/* The tree part of KeyFrame::SetBadFlag (:607-668) for the keyframe of `slot`; call it after corb_covis_erase(slot), as the reference orders it.  The greedy loop: per
 * round every child (ascending id; a child the store does not hold or a bad one is skipped) walks its GetVectorCovisibleKeyFrames() in list order, an entry whose mnId
 * equals a parent candidate's competes with GetWeight, a strict `>` keeps the first best; the winner gets ChangeParent, joins the candidates (which start as the held
 * mpParent) and leaves the set.  What is left goes to the original parent ONLY under the reference's condition `!mspChildrens.empty() && mpParent held` (:658), and
 * `mpParent->EraseChild(this)` and `mbBad = true` sit inside that same `if`: a keyframe whose children were all re-parented, or that had none, is NOT erased from its
 * parent's set and the reference does not mark it bad.  *reference_sets_bad tells which (1: the `if` was entered).  The leftover children stay in the set (the reference
 * does not clear it).  *n_changed = ChangeParent calls made.  CORB_KF_BAD itself stays the caller's to set. */
int corb_covis_reparent_children(CorbCovis* g, int slot, int* n_changed, int* reference_sets_bad);

/* Tracking::UpdateLocalMap (C/src/Tracking.cc:1218-1366): UpdateLocalKeyFrames + UpdateLocalPoints for the current frame = record `slot` of `frames` (the graph's keyframe
 * store or another one).  prev_kf_slots = mvpLocalKeyFrames before the call; kf_slots / mp_slots / mp_ids = mvpLocalKeyFrames / mvpLocalMapPoints after it, as slots of the
 * graph's stores; mp_ids is the local_ids argument of corb_track_search_local_points.  What the reference's words mean here:
 *   walk orders    keyframeCounter, GetChilds() and GetObservations() are pointer-keyed containers in the reference (allocator-dependent order); here every such walk
 *                  is in ASCENDING KEYFRAME ID.  pKFmax is the non-bad voter with the most votes, the smallest id among equals (strict `>`, :1299)
 *   a voter        an observer the graph's keyframe store holds (GetObservations, MapPoint.cc:219-231); other observers are dropped before counting
 *   :1278          a feature whose point resolves to a bad record loses its point IN THE FRAME RECORD; an id that does not resolve is left alone (n_cleared counts)
 *   :1282          an empty counter returns early: the list is prev_kf_slots unchanged, the reference keyframe untouched (ref_slot -1), counter_empty set;
 *                  UpdateLocalPoints still runs on that list.  A non-empty counter whose voters are all bad gives an empty list and no points
 *   :1310-1360     the neighbour walk runs over the voted keyframes only (the end iterator is taken before the pushes), stops when the list holds more than 80 at the
 *                  top of an iteration, pushes per keyframe the first not-yet-included non-bad member of GetBestCovisibilityKeyFrames(10), then the first such child,
 *                  then the parent if not yet included -- and the `break` after pushing a parent LEAVES THE WHOLE WALK (:1356)
 *   marks          mnTrackReferenceForFrame of keyframes and points are per-call; no record but the frame's is written
 *   :1230-1256     UpdateLocalPoints does not test pKF->isBad(): every feature's point that resolves and is not bad, first occurrence in (list order, feature order)
 * CORB_ERR_CAPACITY: more than max_connections distinct voters, or a list beyond kf_cap / mp_cap; detected before anything is written, the frame record's cleared points
 * included.  Without a map-point index, or with an empty slot as the frame or among prev_kf_slots: CORB_ERR_ARG.  One read-back per call: the true counts are not known
 * before it, so 4 bytes per keyframe of kf_cap and 12 per point of mp_cap cross whatever the lists hold, and kf_cap x (feature capacity) sizes the points pass's launch --
 * size the caps for a local map (a hundred keyframes, some thousand points), not for the stores.  Locks: the graph, then each store once as corb_fuse_store does. */
typedef struct CorbLocalMap {
    int32_t n_kf, n_voted, n_mp;    /* local keyframes, the voted ones among them (the front of the list), local map points */
    int32_t ref_slot;               /* pKFmax as a slot, -1: mpReferenceKF unchanged */
    uint64_t ref_id;                /* its mnId, CORB_NO_MAP_POINT if none */
    int32_t counter_empty, n_cleared;
} CorbLocalMap;
int corb_track_update_local_map(CorbCovis* g, CorbKfStore* frames, int slot, const int32_t* prev_kf_slots, int n_prev, int32_t* kf_slots, int kf_cap,
                                int32_t* mp_slots, uint64_t* mp_ids, int mp_cap, CorbLocalMap* out);

/* ---- the map update that follows a global bundle adjustment (RunGlobalBundleAdjustment, corbslam_server/src/GlobalOptimize.cpp:463-532 = corbslam_client/src/
 * LoopClosing.cc:684-753): what corb_ba_solve_store with loop_kf != 0 left in TcwGBA / pos_gba / ba_global_for_kf becomes Tcw / world_pos, and keyframes the solve did
 * not see are corrected through the spanning tree.  "Held" and "non-bad" mean what the section above says; without a map-point index: CORB_ERR_ARG.
 *   mTcwBefGBA     the 256-byte keyframe header has no room for it: it lives in the graph, one 4x4 float per slot, read and written with the two calls below.  A fresh
 *                  graph holds the IDENTITY (the reference leaves the matrix uninitialised, KeyFrame.cc:62)
 *   the walk       the reference's queue, exactly: it starts as origin_slots (mvpKeyFrameOrigins); a pop walks the EXPLICIT child set of the keyframe in ascending id (not
 *                  the parent fields), skips a child the store does not hold, gives a child whose ba_global_for_kf != loop_kf
 *                  TcwGBA = (Tcw(child) * Twc) * TcwGBA(popped) and the mark, pushes EVERY held child, marked or not, then does mTcwBefGBA = Tcw, Tcw = TcwGBA.
 *                  No bad test is made.  So: an unmarked origin is SetPose'd with whatever TcwGBA its record holds; a keyframe listed in two sets (ChangeParent
 *                  leaves the stale entry) is popped twice and ends with mTcwBefGBA == TcwGBA; of two listers of one unmarked child the earlier queue position
 *                  computes its pose; a keyframe no origin reaches keeps Tcw and mTcwBefGBA
 *   queue_cap      bounds the queue, pops included (<= 0: 4 x slots + 64).  The reference does not terminate on a cyclic child set and pops exponentially often on
 *                  stacked diamonds; a walk that would exceed the bound answers CORB_ERR_CAPACITY BEFORE anything is committed (records, graph and *out unchanged)
 *   the points     every slot of the map-point index: a bad point is passed over; ba_global_for_kf == loop_kf: world_pos = pos_gba (n_points_set); else, with the
 *                  reference keyframe held and marked after the walk: Xc = Rcw_bef*p + tcw_bef, p = Rwc*Xc + twc with its mTcwBefGBA and the inverse of its Tcw as they
 *                  stand -- a keyframe the walk never reached contributes its STORED mTcwBefGBA (n_points_moved); else the point is left alone (n_points_skipped).
 *                  Normal and distances are not touched: the reference calls no UpdateNormalAndDepth here
 *   arithmetic     float products as corb_rebase_map_store makes them (exact products summed in double, left to right, one rounding), `A*x + b` one more float add;
 *                  Twc is SetPose's: Rwc = Rcw^T, Ow = -(Rwc*tcw).  Every output is reproducible bit for bit (tests/loopfix_reference.py)
 * n_popped = queue entries in all, n_reached = distinct keyframes among them, n_revisited = n_popped - n_reached, n_propagated = poses composed.
 * Locks: the graph, then each store once as corb_fuse_store does. */
/* CorrectLoop's propagation (GlobalOptimize.cpp:253-338 = LoopClosing.cc:436-522) for mpCurrentKF = cur_slot and mg2oScw = Scw (8 doubles: quaternion x y z w, t, s --
 * the layout corb_optimize_essential_graph takes as S).  The set is GetVectorCovisibleKeyFrames() of cur_slot as corb_covis_query answers it (ids the store does not
 * hold are dropped) plus the current keyframe.
 *   walk order     CorrectedSim3 / NonCorrectedSim3 are pointer-keyed std::maps in the reference (LoopClosing.h:51); here the walk is in ASCENDING KEYFRAME ID, and
 *                  kf_slots[0 .. n) with the two n x 8 arrays come back in that order.  More than cap members: CORB_ERR_CAPACITY with *n set and nothing written
 *   the Sim3s      Tic = Tiw*Twc in float (products as corb_rebase_map_store makes them); Sic = Sim3(Ric, tic, 1); CorrectedSiw = Sic * Scw, for the current keyframe
 *                  Scw itself; NonCorrected = Sim3(Riw, tiw, 1).  The g2o::Sim3 parts are FP64 in the reference's operation order
 *   the points     a map point is corrected ONCE, by the first member in walk order that holds it -- a per-feature id of that record that resolves to a non-bad record; a
 *                  point whose scratch corrected_by_kf equals the current keyframe's id on entry is skipped.  p <- CorrectedSwi.map(Siw.map(p)) in FP64, rounded to
 *                  float; the scratch fields corrected_by_kf = id(cur) and corrected_reference = id(corrector) are written.  These kernels are the first of the library
 *                  to read and write CorbMapPointScratch fields (corb_mp_store_set_scratch says the kernels do not read the scratch: these two are the exception)
 *   :320           UpdateNormalAndDepth is applied when scale_factor > 0 (0: the three fields are left alone, as in corb_ba_solve_store).  It runs in the middle of
 *                  the reference's walk and so meets a mixture of poses: an observer, or the reference keyframe, that belongs to the set and comes BEFORE the
 *                  corrector in walk order has its corrected pose; the corrector itself, every later member and every keyframe outside the set have their old one
 *                  (SetPose at :332 comes after the keyframe's own point loop).  The arithmetic is corb_ba_solve_store's
 *   the poses      Tcw <- [R | t * (1./s)] of CorrectedSiw for every member (:324-332); no bad or fixed test is made, the reference makes none
 *   :337           pKFi->UpdateConnections() reads observations only: the caller follows with ONE corb_covis_update(g, kf_slots, n, 15, ...), whose "as if one after the
 *                  other in list order" rule makes that equal
 * No output depends on the order the device's atomics land in.  Locks: the graph, then each store once as corb_fuse_store does. */
int corb_loop_correct_store(CorbCovis* g, int cur_slot, const double* Scw /* 8 */, float scale_factor, int32_t* kf_slots, double* corrected /* n x 8 */,
                            double* non_corrected /* n x 8 */, int cap, int* n, int* n_points_corrected);
typedef struct CorbGbaPropagation { int32_t n_popped, n_reached, n_propagated, n_revisited, n_points_set, n_points_moved, n_points_skipped; } CorbGbaPropagation;
int corb_gba_propagate_store(CorbCovis* g, const int32_t* origin_slots, int n_origins, uint64_t loop_kf, int queue_cap, CorbGbaPropagation* out);
int corb_covis_set_pose_before_gba(CorbCovis* g, int slot, const float* T /* 16, row-major */);
int corb_covis_get_pose_before_gba(CorbCovis* g, int slot, float* T /* 16 */);

#ifdef __cplusplus
}
#endif
#endif
