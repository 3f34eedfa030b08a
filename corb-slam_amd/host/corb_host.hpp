// corb_host.hpp -- C++ host-side mirror of the reference's operator interface for the hot path, over the
// C-ABI of libcorb_accel.so (include/corb_accel.h).  Header-only, no OpenCV / Eigen / ROS: containers are
// std::vector and the POD structs of the C-ABI.  Same class and method names, argument meaning and
// "error" behaviour as the reference (which has no error path: an empty image yields no keypoints; a
// failure inside the accelerator throws corb::Error instead of silently falling back to the CPU).
//
//   ORB_SLAM2::ORBextractor  (corbslam_client/include/ORBextractor.h:45-114)   -> corb::ORBextractor
//   ORB_SLAM2::ORBmatcher    (corbslam_client/include/ORBmatcher.h:41-107)     -> corb::ORBmatcher
//   ORB_SLAM2::Optimizer     (corbslam_client/include/Optimizer.h:42-46)       -> corb::Optimizer
//   Frame::ComputeStereoMatches (corbslam_client/src/Frame.cc:470-644)          -> corb::StereoFrontend
//   cv::initUndistortRectifyMap + cv::remap of the stereo mains (corbslam_client/Examples/Stereo/stereo_euroc.cc:64-98,136-137) -> corb::StereoRectifier
//
// corb_adapter_opencv.hpp layers the exact cv::/KeyFrame signatures on top of this where OpenCV exists.
#pragma once
#include <corb_accel.h>
#include <corb_stereo_rectify.h>
#include <corb_map_fusion.h>
#include <corb_track_local_map.h>
#include <corb_track_frame.h>
#include <corb_trajectory.h>
#include <corb_loop_detect.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include <cmath>

namespace corb {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what + ": " + corb_last_error()), code(c) {}
};
inline void check(int rc, const char* what) { if (rc != CORB_OK) throw Error(rc, what); }
// The structs of corb_accel.h carry no size fields: the library must have been built from the header this translation unit was compiled against.
// Checked by Warmup() and by every class of this header on its first use (one comparison of a function-local static).
inline void check_abi()
{
    static const int v = corb_abi_version();
    if (v != CORB_ABI_VERSION) throw std::runtime_error("libcorb_accel.so: struct layout version " + std::to_string(v) + ", this program was compiled against " + std::to_string(CORB_ABI_VERSION));
}
// once per process and device at start-up: the per-device workspace lanes are created now, not inside the first bundle adjustment
inline void Warmup(int device = 0) { check_abi(); check(corb_warmup(device), "corb_warmup"); }

using KeyPoint = CorbKeyPoint;                       // bit-identical to cv::KeyPoint as the reference fills it
struct Descriptors { std::vector<uint8_t> data; int rows() const { return (int)(data.size() / 32); } const uint8_t* row(int i) const { return &data[(size_t)i * 32]; } };

class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };       // ORBextractor.h:49 (unused by the reference as well)
    // ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST) + the image size
    // the handle is built for (the reference sizes its pyramid lazily per call; the device arena is static)
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int width, int height, int device = 0)
        : nlevels_(nlevels), width_(width), height_(height)
    {
        check_abi();
        CorbOrbConfig cfg{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, 1, device};
        check(corb_orb_create(&cfg, &h_), "corb_orb_create");
        cap_ = nfeatures + 16 * nlevels + 256;
    }
    ~ORBextractor() { corb_orb_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // void operator()(cv::InputArray image, cv::InputArray mask, std::vector<cv::KeyPoint>&, cv::OutputArray descriptors)
    // (mask is ignored by the reference, ORBextractor.cc:1043)
    void operator()(const uint8_t* image, int width, int height, int stride, std::vector<KeyPoint>& keypoints, Descriptors& descriptors)
    {
        keypoints.resize(cap_); descriptors.data.resize((size_t)cap_ * 32);
        int n = 0;
        check(corb_orb_extract(h_, image, width, height, stride, keypoints.data(), descriptors.data.data(), cap_, &n), "corb_orb_extract");
        keypoints.resize(n); descriptors.data.resize((size_t)n * 32);
    }
    int GetLevels() const { return nlevels_; }
    float GetScaleFactor() const { return table(0)[nlevels_ > 1 ? 1 : 0]; }
    std::vector<float> GetScaleFactors() const { return table(0); }
    std::vector<float> GetInverseScaleFactors() const { return table(1); }
    std::vector<float> GetScaleSigmaSquares() const { return table(2); }
    std::vector<float> GetInverseScaleSigmaSquares() const { return table(3); }
    // mvImagePyramid[level] (public member of the reference, read by Frame::ComputeStereoMatches)
    std::vector<uint8_t> ImagePyramidLevel(int level, int* w, int* h) const
    {
        check(corb_orb_pyramid_level(h_, 0, level, 0, nullptr, 0, w, h), "corb_orb_pyramid_level");
        std::vector<uint8_t> out((size_t)*w * *h);
        check(corb_orb_pyramid_level(h_, 0, level, 0, out.data(), out.size(), w, h), "corb_orb_pyramid_level");
        return out;
    }
    CorbOrb* handle() const { return h_; }
private:
    std::vector<float> table(int which) const
    {
        std::vector<float> t[4]; for (auto& v : t) v.resize(nlevels_);
        check(corb_orb_tables(h_, t[0].data(), t[1].data(), t[2].data(), t[3].data(), nullptr, nullptr), "corb_orb_tables");
        return t[which];
    }
    CorbOrb* h_ = nullptr; int nlevels_, width_, height_, cap_;
};

// Frame::Frame(stereo) hot path: left + right ORBextractor::operator() and Frame::ComputeStereoMatches
class StereoFrontend {
public:
    struct FrameResult { std::vector<KeyPoint> mvKeys, mvKeysRight; Descriptors mDescriptors, mDescriptorsRight; std::vector<float> mvuRight, mvDepth; };
    StereoFrontend(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int width, int height,
                   float fx, float bf, int max_frames = 1, int device = 0) : max_frames_(max_frames)
    {
        CorbStereoConfig cfg{{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, 0, device}, max_frames, fx, bf};
        check(corb_stereo_create(&cfg, &h_), "corb_stereo_create");
        cap_ = nfeatures + 16 * nlevels + 256;
    }
    ~StereoFrontend() { corb_stereo_destroy(h_); }
    void Upload(int frame, const uint8_t* left, const uint8_t* right, int stride) { check(corb_stereo_upload(h_, frame, left, right, stride), "corb_stereo_upload"); }
    // whole batches with one copy each (pinned host memory = DMA): leftRight = per frame the left image then the right image, tightly packed;
    // results strided by Capacity(): keypoints / descriptors of image 2f (left) and 2f+1 (right), mvuRight / mvDepth per frame
    void UploadBatch(int firstFrame, int nFrames, const uint8_t* leftRight) { check(corb_stereo_upload_batch(h_, firstFrame, nFrames, leftRight), "corb_stereo_upload_batch"); }
    int Capacity() const { return corb_orb_capacity(corb_stereo_orb(h_)); }
    void FetchBatch(int firstFrame, int nFrames, KeyPoint* keys, uint8_t* descriptors, int32_t* counts, float* uRight, float* depth, int32_t* nMatched)
    {
        check(corb_orb_fetch_batch(corb_stereo_orb(h_), 2 * firstFrame, 2 * nFrames, keys, descriptors, counts), "corb_orb_fetch_batch");
        check(corb_stereo_fetch_matches_batch(h_, firstFrame, nFrames, uRight, depth, nMatched), "corb_stereo_fetch_matches_batch");
    }
    void Run(int n_frames) { check(corb_stereo_run(h_, n_frames), "corb_stereo_run"); }
    // Frame::Frame(stereo) (Frame.cc:61-117) as ONE call (corb_stereo_frames): nFrames x {left, right} images tightly packed in, nFrames result blocks out
    // (page-locked buffers from corb_pinned_alloc make both transfers DMA); one synchronisation.  FromBlock() copies a block into the containers of Fetch().
    CorbStereoFrameLayout FrameLayout() const { CorbStereoFrameLayout l; check(corb_stereo_frame_layout(h_, &l), "corb_stereo_frame_layout"); return l; }
    void Frames(int nFrames, const uint8_t* leftRight, void* resultBlocks, CorbStereoFrameTiming* timing = nullptr) { check(corb_stereo_frames(h_, nFrames, leftRight, resultBlocks, timing), "corb_stereo_frames"); }
    static FrameResult FromBlock(const CorbStereoFrameLayout& l, const void* block)
    {
        const uint8_t* b = static_cast<const uint8_t*>(block); const int32_t* hd = reinterpret_cast<const int32_t*>(b);
        FrameResult r; const size_t nl = (size_t)hd[0], nr = (size_t)hd[1];
        r.mvKeys.assign(reinterpret_cast<const KeyPoint*>(b + l.off_kp_left), reinterpret_cast<const KeyPoint*>(b + l.off_kp_left) + nl);
        r.mvKeysRight.assign(reinterpret_cast<const KeyPoint*>(b + l.off_kp_right), reinterpret_cast<const KeyPoint*>(b + l.off_kp_right) + nr);
        r.mDescriptors.data.assign(b + l.off_desc_left, b + l.off_desc_left + 32 * nl); r.mDescriptorsRight.data.assign(b + l.off_desc_right, b + l.off_desc_right + 32 * nr);
        r.mvuRight.assign(reinterpret_cast<const float*>(b + l.off_u_right), reinterpret_cast<const float*>(b + l.off_u_right) + nl);
        r.mvDepth.assign(reinterpret_cast<const float*>(b + l.off_depth), reinterpret_cast<const float*>(b + l.off_depth) + nl);
        return r;
    }
    CorbStereo* handle() const { return h_; }
    void Sync() { check(corb_stereo_sync(h_), "corb_stereo_sync"); }
    FrameResult Fetch(int frame)
    {
        FrameResult r; int n = 0, nm = 0;
        auto get = [&](int slot, std::vector<KeyPoint>& k, Descriptors& d) {
            k.resize(cap_); d.data.resize((size_t)cap_ * 32);
            check(corb_orb_fetch(corb_stereo_orb(h_), slot, k.data(), d.data.data(), cap_, &n), "corb_orb_fetch");
            k.resize(n); d.data.resize((size_t)n * 32);
        };
        get(2 * frame, r.mvKeys, r.mDescriptors); get(2 * frame + 1, r.mvKeysRight, r.mDescriptorsRight);
        r.mvuRight.resize(cap_); r.mvDepth.resize(cap_);
        check(corb_stereo_fetch_matches(h_, frame, r.mvuRight.data(), r.mvDepth.data(), cap_, &n, &nm), "corb_stereo_fetch_matches");
        r.mvuRight.resize(n); r.mvDepth.resize(n);
        return r;
    }
private:
    CorbStereo* h_ = nullptr; int max_frames_, cap_;
};

// The rectification the reference's stereo mains for unrectified cameras do on the host before TrackStereo (Examples/Stereo/stereo_euroc.cc:64-98,136-137;
// Examples/ROS/ORB_SLAM2/src/ros_stereo.cc:82-107,161-162), in front of a StereoFrontend (include/corb_stereo_rectify.h).  Constructed from the eight matrices of
// the settings file, row-major doubles: K, R 3x3, P 3x4, D of up to 8 coefficients (k1, k2, p1, p2, k3, k4, k5, k6).  Destroy it before its front-end.
class StereoRectifier {
public:
    StereoRectifier(StereoFrontend& frontend, const std::vector<double>& K_l, const std::vector<double>& D_l, const std::vector<double>& R_l, const std::vector<double>& P_l,
                    const std::vector<double>& K_r, const std::vector<double>& D_r, const std::vector<double>& R_r, const std::vector<double>& P_r, int rawWidth, int rawHeight)
    {
        check_abi();
        CorbRectifyConfig cfg{};
        cfg.raw_width = rawWidth; cfg.raw_height = rawHeight;
        auto fill = [](double* dst, size_t n, const std::vector<double>& v, bool exact) {
            if (exact ? v.size() != n : v.size() > n) throw std::invalid_argument("corb::StereoRectifier: a calibration matrix of the wrong size");
            std::copy(v.begin(), v.end(), dst);
        };
        fill(cfg.left.K, 9, K_l, true); fill(cfg.left.D, 8, D_l, false); fill(cfg.left.R, 9, R_l, true); fill(cfg.left.P, 12, P_l, true);
        fill(cfg.right.K, 9, K_r, true); fill(cfg.right.D, 8, D_r, false); fill(cfg.right.R, 9, R_r, true); fill(cfg.right.P, 12, P_r, true);
        check(corb_rect_create(&cfg, frontend.handle(), &h_), "corb_rect_create");
    }
    ~StereoRectifier() { corb_rect_destroy(h_); }
    StereoRectifier(const StereoRectifier&) = delete;
    StereoRectifier& operator=(const StereoRectifier&) = delete;
    // M1 / M2 of eye 0 (left) / 1 (right): height x width floats each
    void Maps(int eye, float* mapX, float* mapY) const { check(corb_rect_maps(h_, eye, mapX, mapY), "corb_rect_maps"); }
    void SetMaps(int eye, const float* mapX, const float* mapY) { check(corb_rect_set_maps(h_, eye, mapX, mapY), "corb_rect_set_maps"); }
    // cv::remap of both raw images of every frame (per frame the raw left image then the raw right image, tightly packed); then the front-end's Run / Sync / Fetch
    void UploadBatch(int firstFrame, int nFrames, const uint8_t* rawLeftRight) { check(corb_rect_upload_batch(h_, firstFrame, nFrames, rawLeftRight), "corb_rect_upload_batch"); }
    // StereoFrontend::Frames for raw input: the same result blocks (StereoFrontend::FrameLayout, StereoFrontend::FromBlock)
    void Frames(int nFrames, const uint8_t* rawLeftRight, void* resultBlocks, CorbStereoFrameTiming* timing = nullptr) { check(corb_rect_frames(h_, nFrames, rawLeftRight, resultBlocks, timing), "corb_rect_frames"); }
    CorbRect* handle() const { return h_; }
private:
    CorbRect* h_ = nullptr;
};

// Frame::Frame(RGB-D) / Frame::Frame(monocular) (Frame.cc:119-228) with Tracking::GrabImageRGBD / GrabImageMonocular's input conversions (Tracking.cc:206-264).
// cfg: the settings file's camera and ORB values (CorbCameraConfig); one frame of input = colour (or grey) image, then the depth image (RGB-D), tightly packed.
class RgbdFrontend {
public:
    struct FrameResult { std::vector<KeyPoint> mvKeys, mvKeysUn; Descriptors mDescriptors; std::vector<float> mvuRight, mvDepth; float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0; };
    explicit RgbdFrontend(const CorbCameraConfig& cfg)
    {
        check(corb_rgbd_create(&cfg, &h_), "corb_rgbd_create");
        check(corb_rgbd_frame_layout(h_, &lay_), "corb_rgbd_frame_layout");
        check(corb_rgbd_image_bounds(h_, bounds_), "corb_rgbd_image_bounds");
    }
    ~RgbdFrontend() { corb_rgbd_destroy(h_); }
    RgbdFrontend(const RgbdFrontend&) = delete;
    RgbdFrontend& operator=(const RgbdFrontend&) = delete;
    const CorbRgbdFrameLayout& FrameLayout() const { return lay_; }
    int InputBytes() const { return lay_.input_bytes; }
    int Capacity() const { return lay_.capacity; }
    // Frame::ComputeImageBounds of the calibration: {mnMinX, mnMaxX, mnMinY, mnMaxY}
    void Bounds(float out[4]) const { for (int i = 0; i < 4; i++) out[i] = bounds_[i]; }
    // the per-frame call (corb_rgbd_frames): nFrames inputs in, nFrames result blocks of FrameLayout().frame_bytes out, one synchronisation
    void Frames(int nFrames, const uint8_t* input, void* resultBlocks, CorbStereoFrameTiming* timing = nullptr) { check(corb_rgbd_frames(h_, nFrames, input, resultBlocks, timing), "corb_rgbd_frames"); }
    FrameResult FromBlock(const void* block) const
    {
        const uint8_t* b = static_cast<const uint8_t*>(block);
        const size_t n = (size_t)reinterpret_cast<const int32_t*>(b)[0];
        FrameResult r;
        r.mvKeys.assign(reinterpret_cast<const KeyPoint*>(b + lay_.off_keys), reinterpret_cast<const KeyPoint*>(b + lay_.off_keys) + n);
        r.mvKeysUn.assign(reinterpret_cast<const KeyPoint*>(b + lay_.off_keys_un), reinterpret_cast<const KeyPoint*>(b + lay_.off_keys_un) + n);
        r.mDescriptors.data.assign(b + lay_.off_desc, b + lay_.off_desc + 32 * n);
        r.mvuRight.assign(reinterpret_cast<const float*>(b + lay_.off_u_right), reinterpret_cast<const float*>(b + lay_.off_u_right) + n);
        r.mvDepth.assign(reinterpret_cast<const float*>(b + lay_.off_depth), reinterpret_cast<const float*>(b + lay_.off_depth) + n);
        r.mnMinX = bounds_[0]; r.mnMaxX = bounds_[1]; r.mnMinY = bounds_[2]; r.mnMaxY = bounds_[3];
        return r;
    }
    // one frame: Frames(1, ...) into a block this object keeps
    FrameResult ProcessFrame(const uint8_t* input)
    {
        block_.resize((size_t)lay_.frame_bytes);
        Frames(1, input, block_.data());
        return FromBlock(block_.data());
    }
    // batches: one upload + conversion kernel, an asynchronous run of frames 0 .. n-1, strided results (Capacity() entries per frame)
    void UploadBatch(int firstFrame, int nFrames, const uint8_t* input) { check(corb_rgbd_upload_batch(h_, firstFrame, nFrames, input), "corb_rgbd_upload_batch"); }
    void Run(int nFrames) { check(corb_rgbd_run(h_, nFrames), "corb_rgbd_run"); }
    void Sync() { check(corb_rgbd_sync(h_), "corb_rgbd_sync"); }
    void FetchBatch(int firstFrame, int nFrames, KeyPoint* keys, KeyPoint* keysUn, uint8_t* descriptors, float* uRight, float* depth, int32_t* counts)
    {
        check(corb_rgbd_fetch_batch(h_, firstFrame, nFrames, keys, keysUn, descriptors, uRight, depth, counts), "corb_rgbd_fetch_batch");
    }
    CorbRgbd* handle() const { return h_; }
private:
    CorbRgbd* h_ = nullptr;
    CorbRgbdFrameLayout lay_{};
    float bounds_[4] = {0, 0, 0, 0};
    std::vector<uint8_t> block_;
};

// DBoW2::FeatureVector = std::map<NodeId, std::vector<unsigned>>, flattened in ascending node order
struct FeatureVector {
    std::vector<uint32_t> node_id, idx; std::vector<int32_t> offset{0};
    void add(uint32_t node, const std::vector<unsigned>& features) { node_id.push_back(node); idx.insert(idx.end(), features.begin(), features.end()); offset.push_back((int32_t)idx.size()); }
    CorbFeatVec c() const { return CorbFeatVec{(int32_t)node_id.size(), node_id.data(), offset.data(), idx.data()}; }
};

// what the matchers read from a KeyFrame / Frame
struct FeatureSet {
    Descriptors desc; std::vector<KeyPoint> keysUn; std::vector<float> uRight;
    std::vector<uint8_t> hasGoodMapPoint;           // vpMapPoints[i] && !isBad()
    FeatureVector featVec;
    std::vector<float> angles() const { std::vector<float> a(keysUn.size()); for (size_t i = 0; i < a.size(); i++) a[i] = keysUn[i].angle; return a; }
};

class ORBmatcher {
public:
    static constexpr int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;       // ORBmatcher.cc:37-39
    ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0) : mfNNratio(nnratio), mbCheckOrientation(checkOri), device_(device) {}
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b, int device = 0) { int32_t d = 0; check(corb_descriptor_distance(a, b, 1, &d, device), "corb_descriptor_distance"); return d; }
    // int SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches): matches[iF] = KF feature index or -1
    int SearchByBoW(const FeatureSet& kf, const FeatureSet& frame, std::vector<int32_t>& matches) const { return bow(0, kf, frame, matches); }
    int SearchByBoWInServer(const FeatureSet& kf, const FeatureSet& f, std::vector<int32_t>& matches) const { return bow(0, kf, f, matches); }
    // int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12): matches12[i1] = idx2 or -1
    int SearchByBoW_KF(const FeatureSet& kf1, const FeatureSet& kf2, std::vector<int32_t>& matches12) const { return bow(1, kf1, kf2, matches12); }
    // int SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12, vector<pair<size_t,size_t>>&, bool bOnlyStereo)
    int SearchForTriangulation(const FeatureSet& kf1, const FeatureSet& kf2, const float F12[9], float ex, float ey,
                               const std::vector<float>& scaleFactors2, const std::vector<float>& levelSigma2_2,
                               std::vector<std::pair<size_t, size_t>>& vMatchedPairs, bool bOnlyStereo) const
    {
        CorbTriSide a{kf1.desc.data.data(), kf1.keysUn.data(), kf1.uRight.data(), kf1.hasGoodMapPoint.data(), (int32_t)kf1.keysUn.size(), kf1.featVec.c()};
        CorbTriSide b{kf2.desc.data.data(), kf2.keysUn.data(), kf2.uRight.data(), kf2.hasGoodMapPoint.data(), (int32_t)kf2.keysUn.size(), kf2.featVec.c()};
        std::vector<int32_t> pairs(2 * kf1.keysUn.size() + 2); int n = 0;
        check(corb_search_for_triangulation(&a, &b, F12, ex, ey, scaleFactors2.data(), levelSigma2_2.data(), (int)scaleFactors2.size(),
                                            bOnlyStereo, mbCheckOrientation, pairs.data(), &n, device_), "corb_search_for_triangulation");
        vMatchedPairs.clear();
        for (int i = 0; i < n; i++) vMatchedPairs.emplace_back((size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]);
        return n;
    }
    // int SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, float th) (ORBmatcher.cc:45-131): `tracked` holds the
    // points with mbTrackInView (their cached isInFrustum() outputs); matches[iF] = index into `tracked` or -1
    int SearchByProjection(const CorbFrameView& F, const std::vector<CorbTrackedPoint>& tracked, const uint8_t* pointDescriptors, float th,
                           std::vector<int32_t>& matches) const
    {
        matches.assign(F.n > 0 ? F.n : 1, -1); int n = 0;
        check(corb_search_by_projection_map(&F, tracked.data(), pointDescriptors, (int)tracked.size(), th, mfNNratio, matches.data(), &n, device_), "corb_search_by_projection_map");
        matches.resize(F.n);
        return n;
    }
    // int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, float th, bool bMono) (ORBmatcher.cc:1470-1614)
    int SearchByProjection(const CorbFrameView& Cur, const float Tcw[16], const float Tlw[16], float fx, float fy, float cx, float cy, float mbf, float mb,
                           const std::vector<CorbLastPoint>& last, const uint8_t* lastDescriptors, float th, bool bMono, std::vector<int32_t>& matches) const
    {
        matches.assign(Cur.n > 0 ? Cur.n : 1, -1); int n = 0;
        check(corb_search_by_projection_frame(&Cur, Tcw, Tlw, fx, fy, cx, cy, mbf, mb, last.data(), lastDescriptors, (int)last.size(), th, bMono ? 1 : 0,
                                              mbCheckOrientation ? 1 : 0, matches.data(), &n, device_), "corb_search_by_projection_frame");
        matches.resize(Cur.n);
        return n;
    }

    // int SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1616-1744):
    // points[i] = the MapPoint of keyframe feature i (valid = non-NULL && !isBad() && !sAlreadyFound.count()); matches[iF] = i or -1
    int SearchByProjection(const CorbKeyFrameView& CurrentFrame, const std::vector<uint8_t>& hasMapPoint, const float Tcw[16],
                           const std::vector<CorbMapPointView>& points, const uint8_t* pointDescriptors, float th, int ORBdist, std::vector<int32_t>& matches) const
    {
        matches.assign(CurrentFrame.n > 0 ? CurrentFrame.n : 1, -1); int n = 0;
        check(corb_search_by_projection_reloc(&CurrentFrame, hasMapPoint.data(), Tcw, points.data(), pointDescriptors, (int)points.size(), th, ORBdist,
                                              mbCheckOrientation ? 1 : 0, matches.data(), &n, device_), "corb_search_by_projection_reloc");
        matches.resize(CurrentFrame.n);
        return n;
    }
    // int SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12, int windowSize) (ORBmatcher.cc:540-655):
    // prevMatched = vbPrevMatched as n(F1) x 2 floats, read and written; matches12[i1] = feature of F2 or -1
    int SearchForInitialization(const CorbFrameView& F1, const CorbFrameView& F2, std::vector<float>& prevMatched, std::vector<int32_t>& matches12, int windowSize = 10) const
    {
        matches12.assign(F1.n > 0 ? F1.n : 1, -1); int n = 0;
        prevMatched.resize((size_t)2 * (F1.n > 0 ? F1.n : 1));
        check(corb_search_for_initialization(&F1, &F2, prevMatched.data(), windowSize, mfNNratio, mbCheckOrientation ? 1 : 0, matches12.data(), &n, device_), "corb_search_for_initialization");
        matches12.resize(F1.n); prevMatched.resize((size_t)2 * F1.n);
        return n;
    }
    // int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, int th) (ORBmatcher.cc:425-538):
    // hasMatch[idx] = vpMatched[idx] != NULL on entry; points[i].valid = !isBad() && !spAlreadyFound.count(); matches[idx] = i (the point written into vpMatched[idx]) or -1
    int SearchByProjection(const CorbKeyFrameView& pKF, const std::vector<uint8_t>& hasMatch, const float Scw[16], const std::vector<CorbMapPointView>& points,
                           const uint8_t* pointDescriptors, int th, std::vector<int32_t>& matches) const
    {
        matches.assign(pKF.n > 0 ? pKF.n : 1, -1); int n = 0;
        check(corb_search_by_projection_scw(&pKF, hasMatch.data(), Scw, points.data(), pointDescriptors, (int)points.size(), (float)th, matches.data(), &n, device_),
              "corb_search_by_projection_scw");
        matches.resize(pKF.n);
        return n;
    }
    // int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th) (:960-1116): bestIdx[i] = feature of pKF point i fuses into, or -1.
    // The caller then runs the reference's tail per point: Replace() by observation count if pKF->GetMapPoint(bestIdx) exists, else AddObservation/AddMapPoint.
    int Fuse(const CorbKeyFrameView& pKF, const float Tcw[16], const float Ow[3], const std::vector<CorbMapPointView>& points, const uint8_t* pointDescriptors,
             float th, std::vector<int32_t>& bestIdx) const
    { return fuse(pKF, Tcw, Ow, 0, points, pointDescriptors, th, bestIdx); }
    // int Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, th, vector<MapPoint*>& vpReplacePoint) (:1118-1241)
    int Fuse(const CorbKeyFrameView& pKF, const float Scw[16], const std::vector<CorbMapPointView>& points, const uint8_t* pointDescriptors,
             float th, std::vector<int32_t>& bestIdx) const
    { return fuse(pKF, Scw, nullptr, 1, points, pointDescriptors, th, bestIdx); }
    // int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, s12, R12, t12, th) (:1244-1468): matches12[i1] = feature of KF2 or -1
    int SearchBySim3(const CorbKeyFrameView& kf1, const CorbKeyFrameView& kf2, const float T1w[16], const float T2w[16],
                     const std::vector<CorbMapPointView>& points1, const uint8_t* desc1, const std::vector<CorbMapPointView>& points2, const uint8_t* desc2,
                     float s12, const float R12[9], const float t12[3], float th, std::vector<int32_t>& matches12) const
    {
        matches12.assign(kf1.n > 0 ? kf1.n : 1, -1); int n = 0;
        check(corb_search_by_sim3(&kf1, &kf2, T1w, T2w, points1.data(), desc1, points2.data(), desc2, s12, R12, t12, th, matches12.data(), &n, device_), "corb_search_by_sim3");
        matches12.resize(kf1.n);
        return n;
    }

private:
    int fuse(const CorbKeyFrameView& K, const float* T, const float* Ow, int sim3, const std::vector<CorbMapPointView>& pts, const uint8_t* desc, float th,
             std::vector<int32_t>& bestIdx) const
    {
        bestIdx.assign(pts.size() ? pts.size() : 1, -1); std::vector<int32_t> bestDist(bestIdx.size()); int n = 0;
        check(corb_fuse(&K, T, Ow, sim3, pts.data(), desc, (int)pts.size(), th, bestIdx.data(), bestDist.data(), &n, device_), "corb_fuse");
        bestIdx.resize(pts.size());
        return n;
    }
    int bow(int variant, const FeatureSet& A, const FeatureSet& B, std::vector<int32_t>& out) const
    {
        std::vector<float> a1 = A.angles(), a2 = B.angles();
        std::vector<uint8_t> ones(B.keysUn.size(), 1);
        CorbBowSide a{A.desc.data.data(), a1.data(), A.hasGoodMapPoint.data(), (int32_t)A.keysUn.size(), A.featVec.c()};
        CorbBowSide b{B.desc.data.data(), a2.data(), variant == 1 ? B.hasGoodMapPoint.data() : ones.data(), (int32_t)B.keysUn.size(), B.featVec.c()};
        out.assign(variant == 0 ? B.keysUn.size() : A.keysUn.size(), -1);
        int n = 0;
        check(corb_search_by_bow(variant, &a, &b, mfNNratio, mbCheckOrientation, out.data(), &n, device_), "corb_search_by_bow");
        return n;
    }
    float mfNNratio; bool mbCheckOrientation; int device_;
};

class Optimizer {
public:
    struct Graph {                                  // what Optimizer::BundleAdjustment reads from KeyFrames / MapPoints
        std::vector<float> Tcw;                     // K x 16, pKF->GetPose()
        std::vector<uint8_t> kfFixed;               // pKF->mnId==1 || pKF->getFixed()
        std::vector<float> worldPos;                // M x 3, pMP->GetWorldPos()
        std::vector<uint8_t> mpFixed;               // pMP->getFixed()
        std::vector<CorbBAEdge> observations;       // one per (MapPoint, KeyFrame) observation
        float fx = 0, fy = 0, cx = 0, cy = 0, bf = 0;  // shared camera (used when intr is empty)
        std::vector<float> intr;                    // K x 5: pKF->fx, fy, cx, cy, mbf of every keyframe (e->fx = pKF->fx ..., Optimizer.cc:160-163, 189-193)
        const float* intrPtr() const { return intr.empty() ? nullptr : intr.data(); }
    };
    // static void GlobalBundleAdjustemnt(Cache*, int nIterations=5, bool* pbStopFlag=NULL, unsigned long nLoopKF=0, bool bRobust=true)
    // (sic -- the reference's spelling, Optimizer.h:45).  The caller applies the nLoopKF write-back policy
    // (SetPose/SetWorldPos when nLoopKF==0, else mTcwGBA/mPosGBA; Optimizer.cc:226-262) from the returned arrays.
    static CorbBAResult GlobalBundleAdjustemnt(const Graph& g, std::vector<float>& TcwOut, std::vector<float>& posOut,
                                               int nIterations = 5, volatile int* pbStopFlag = nullptr, bool bRobust = true, int device = 0)
    { return BundleAdjustment(g, TcwOut, posOut, nIterations, pbStopFlag, bRobust, device); }
    static CorbBAResult BundleAdjustment(const Graph& g, std::vector<float>& TcwOut, std::vector<float>& posOut,
                                         int nIterations, volatile int* pbStopFlag, bool bRobust, int device = 0)
    {
        CorbBAProblem p{(int32_t)(g.Tcw.size() / 16), (int32_t)(g.worldPos.size() / 3), (int32_t)g.observations.size(), g.Tcw.data(), g.kfFixed.data(),
                        g.worldPos.data(), g.mpFixed.data(), g.observations.data(), g.fx, g.fy, g.cx, g.cy, g.bf, g.intrPtr()};
        TcwOut.resize(g.Tcw.size()); posOut.resize(g.worldPos.size());
        CorbBAResult r{}; r.poses = TcwOut.data(); r.points = posOut.data();
        check(corb_ba_solve(&p, nIterations, bRobust, pbStopFlag, &r, device), "corb_ba_solve");
        return r;
    }

    // void LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Cache* pCache) (Optimizer.cc:487-838): the graph holds the local
    // keyframes (free), the fixed keyframes and the local map points; vToErase[i] = observation i failed the chi2 / depth test
    // after the second optimize().  The caller erases those observations and writes the estimates back (Optimizer.cc:799-837).
    static CorbBAResult LocalBundleAdjustment(const Graph& g, std::vector<float>& TcwOut, std::vector<float>& posOut, std::vector<uint8_t>& vToErase,
                                              volatile int* pbStopFlag = nullptr, int device = 0)
    {
        const float hm = std::sqrt(5.991f), hs = std::sqrt(7.815f);
        const CorbBAStage st[2] = { {5, 1, 5.991f, 7.815f, 1, 0, 0, 0, 0, hm, hs}, {10, 0, 5.991f, 7.815f, 1, 0, 1, 0, 0, hm, hs} };   // final test: every edge (allow_reactivate)
        return staged(g, st, 2, TcwOut, posOut, vToErase, pbStopFlag, device);
    }

    // int PoseOptimization(Frame* pFrame) (Optimizer.cc:272-485): Tcw in/out, mvbOutlier out, returns nInitialCorrespondences - nBad.
    // One observation per matched MapPoint: world position, mvKeysUn[i].pt, mvuRight[i] (<0 = monocular), mvInvLevelSigma2[octave].
    struct FrameObservations { std::vector<float> worldPos, u, v, uRight, invSigma2; float fx, fy, cx, cy, bf; };
    static int PoseOptimization(float Tcw[16], const FrameObservations& f, std::vector<uint8_t>& mvbOutlier, int device = 0)
    {
        CorbPoseOptFrame F{Tcw, (int32_t)f.u.size(), f.worldPos.data(), f.u.data(), f.v.data(), f.uRight.data(), f.invSigma2.data(), f.fx, f.fy, f.cx, f.cy, f.bf};
        mvbOutlier.assign(f.u.size() ? f.u.size() : 1, 0);
        uint8_t* op = mvbOutlier.data(); float out[16]; int32_t ninl = 0;
        check(corb_pose_optimization_batch(&F, 1, out, &op, &ninl, device), "corb_pose_optimization_batch");
        mvbOutlier.resize(f.u.size());
        for (int i = 0; i < 16; i++) Tcw[i] = out[i];
        return ninl;
    }

    // int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, float th2, bool bFixScale) (Optimizer.cc:1119-1311).
    // One entry per correspondence the reference turns into an edge pair (pMP1, pMP2 good, i2 >= 0): camera-frame points, keypoints, sigmas.
    struct Sim3Correspondences { std::vector<float> P3D1c, P3D2c, obs1, obs2, invSigma2_1, invSigma2_2; float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2; };
    // R12 (row-major 3x3), t12, s12 = g2oS12 in / out; removed[i] = 1 -> vpMatches1[vnIndexEdge[i]] = NULL; returns nIn
    static int OptimizeSim3(const Sim3Correspondences& c, double R12[9], double t12[3], double& s12, float th2, bool bFixScale, std::vector<uint8_t>& removed, int device = 0)
    {
        CorbSim3Problem P{(int32_t)c.invSigma2_1.size(), c.P3D1c.data(), c.P3D2c.data(), c.obs1.data(), c.obs2.data(), c.invSigma2_1.data(), c.invSigma2_2.data(),
                          c.fx1, c.fy1, c.cx1, c.cy1, c.fx2, c.fy2, c.cx2, c.cy2};
        removed.assign(P.n ? P.n : 1, 0); uint8_t* rp = removed.data(); int32_t nIn = 0;
        check(corb_optimize_sim3(&P, 1, R12, t12, &s12, th2, bFixScale ? 1 : 0, &rp, &nIn, nullptr, device), "corb_optimize_sim3");
        removed.resize(P.n);
        return nIn;
    }

    // void OptimizeEssentialGraph(Cache*, KeyFrame* pLoopKF, KeyFrame* pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale) (Optimizer.cc:840-1117).
    // The caller flattens lines 866-1037: one Sim3 (quaternion x y z w, t, s) per keyframe, fixed flags, EdgeSim3 list (vertex 0, vertex 1, Sji).
    struct EssentialGraph { std::vector<double> S; std::vector<uint8_t> fixed; std::vector<int32_t> vi, vj; std::vector<double> Sji;
                            std::vector<int32_t> pointRef; std::vector<float> points; };
    // S updated in place; TiwOut = K x 16 corrected SE3 poses [R | t/s]; g.points corrected through their reference keyframe
    static int OptimizeEssentialGraph(EssentialGraph& g, std::vector<float>& TiwOut, bool bFixScale, int nIterations = 20, int device = 0)
    {
        const int K = (int)(g.S.size() / 8); TiwOut.resize((size_t)16 * K); int32_t its = 0;
        check(corb_optimize_essential_graph(K, g.S.data(), g.fixed.data(), (int)g.vi.size(), g.vi.data(), g.vj.data(), g.Sji.data(), nIterations, bFixScale ? 1 : 0,
                                            TiwOut.data(), (int)g.pointRef.size(), g.pointRef.data(), g.points.data(), nullptr, &its, device), "corb_optimize_essential_graph");
        return its;
    }

private:
    static CorbBAResult staged(const Graph& g, const CorbBAStage* st, int n, std::vector<float>& TcwOut, std::vector<float>& posOut, std::vector<uint8_t>& outlier,
                               volatile int* pbStopFlag, int device)
    {
        CorbBAProblem p{(int32_t)(g.Tcw.size() / 16), (int32_t)(g.worldPos.size() / 3), (int32_t)g.observations.size(), g.Tcw.data(), g.kfFixed.data(),
                        g.worldPos.data(), g.mpFixed.data(), g.observations.data(), g.fx, g.fy, g.cx, g.cy, g.bf, g.intrPtr()};
        TcwOut.resize(g.Tcw.size()); posOut.resize(g.worldPos.size()); outlier.assign(g.observations.size() ? g.observations.size() : 1, 0);
        CorbBAResult r{}; r.poses = TcwOut.data(); r.points = posOut.data();
        check(corb_ba_solve_staged(&p, st, n, pbStopFlag, &r, outlier.data(), device, nullptr), "corb_ba_solve_staged");
        outlier.resize(g.observations.size());
        return r;
    }
};

// MapPoint::ComputeDistinctiveDescriptors for a batch (MapPoint.cc:337-402): bestRow[p] relative to offset[p]
inline std::vector<int32_t> ComputeDistinctiveDescriptors(const std::vector<uint8_t>& stackedDescriptors, const std::vector<int32_t>& offset, int device = 0)
{
    std::vector<int32_t> best(offset.size() > 1 ? offset.size() - 1 : 1);
    check(corb_distinctive_descriptors(stackedDescriptors.data(), offset.data(), (int)offset.size() - 1, best.data(), device), "corb_distinctive_descriptors");
    best.resize(offset.size() - 1);
    return best;
}
// MapFusion::insertServerMapToGlobleMap arithmetic (S/src/MapFusion.cpp:622-658): Tcw <- Tcw * To2n, p <- Rwc (p - tcw), in place
inline void RebaseMap(const float To2n[16], std::vector<float>& Tcw, std::vector<float>& worldPos, int device = 0)
{ check(corb_rebase_map(To2n, Tcw.data(), (int)(Tcw.size() / 16), worldPos.data(), (int)(worldPos.size() / 3), device), "corb_rebase_map"); }

// iterate()'s loop (C/src/PnPsolver.cc:227-300) as a function of what corb_pnp_ransac returns for one problem -- the one C++ statement of the replay rule (Python:
// pnp_replay).  counts = c_i of the n_counts evaluated hypotheses, records = the call's records (all n_records of them), m = ransac_min_inliers, cap = ransac_max_its,
// s = mnIterations before the call.  The call returns at the first i >= s with c_i >= m whose last record at or before i has refine_ok, else at
// max(cap, s + nIterations) -- or where the evaluated hypotheses end -- with bNoMore and the last record's unrefined pose, if there is one.
struct PnPReplay { enum Kind { None, Best, Refined } kind; int record; int iterations; };
inline PnPReplay pnp_replay(const int32_t* counts, int n_counts, const CorbPnPRansacRecord* records, int n_records, int m, int cap, int s, int nIterations)
{
    const int end = std::min(std::max(cap, s + std::max(nIterations, 0)), n_counts);
    int b = -1;
    for (int i = 0; i < end; i++) {
        if (b + 1 < n_records && records[b + 1].iteration - 1 == i) b++;
        if (i >= s && counts[i] >= m && b >= 0 && records[b].refine_ok) return {PnPReplay::Refined, b, i + 1};
    }
    return {b >= 0 ? PnPReplay::Best : PnPReplay::None, b, std::max(end, s)};
}
// ---- map-fusion detection for a whole submap (include/corb_map_fusion.h).  This header holds no mirror class of the keyframe database or of the record stores (the
// database's class with the reference's signatures is corb::KeyFrameDatabase of corb_adapter_orbslam.hpp, whose DetectMapFusionCandidatesFromDB(vector) calls DetectBatch
// below; the stores are plain handles), so
// the three calls are mirrored here as functions on the handles, sized and cut as the Python harness sizes and cuts them. ----
struct CandidateLists { std::vector<int32_t> offset, cand; };      // cand[offset[i] .. offset[i + 1]) = the candidates of query i
inline CandidateLists DetectBatch(CorbKfDb* db, int kind, const std::vector<int32_t>& entries, const std::vector<uint64_t>& ids, int cap)
{
    if (entries.size() != ids.size()) throw Error(CORB_ERR_ARG, "DetectBatch: entries and ids differ in length");
    CandidateLists o; o.offset.assign(entries.size() + 1, 0); o.cand.assign((size_t)std::max(cap, 1), 0);
    int n = 0;
    check(corb_kfdb_detect_batch(db, kind, entries.data(), ids.data(), (int)entries.size(), o.offset.data(), o.cand.data(), cap, &n), "corb_kfdb_detect_batch");
    o.cand.resize((size_t)n);
    return o;
}
struct BowMatches { int stride = 0; std::vector<int32_t> match, count; };      // row p: match[p * stride ..], -1 behind the row's length
inline BowMatches SearchByBoWSlotsBatch(int variant, CorbKfStore* a, const std::vector<int32_t>& slotsA, CorbKfStore* b, const std::vector<int32_t>& slotsB, float nnratio,
                                        bool checkOrientation, int stride)
{
    if (slotsA.size() != slotsB.size()) throw Error(CORB_ERR_ARG, "SearchByBoWSlotsBatch: the slot lists differ in length");
    BowMatches o; o.stride = stride; o.match.assign(std::max<size_t>(slotsA.size() * (size_t)stride, 1), -1); o.count.assign(std::max<size_t>(slotsA.size(), 1), 0);
    check(corb_search_by_bow_slots_batch(variant, a, slotsA.data(), b, slotsB.data(), (int)slotsA.size(), nnratio, checkOrientation ? 1 : 0, stride, o.match.data(), o.count.data()),
          "corb_search_by_bow_slots_batch");
    o.count.resize(slotsA.size());
    return o;
}
struct FusionCandidates { std::vector<int32_t> rowOffset; std::vector<CorbFusionRow> rows; std::vector<uint64_t> ids; };
inline FusionCandidates MapFusionCandidates(CorbKfDb* db, CorbKfStore* sub, const std::vector<int32_t>& querySlots, const std::vector<int32_t>& queryEntries,
                                            const std::vector<uint64_t>& queryIds, CorbKfStore* global, const std::vector<int32_t>& entrySlot, int capRows, int64_t capIds,
                                            float nnratio = 0.75f, bool checkOrientation = true, int minMatches = 15)
{
    if (querySlots.size() != queryEntries.size() || querySlots.size() != queryIds.size()) throw Error(CORB_ERR_ARG, "MapFusionCandidates: the query lists differ in length");
    FusionCandidates o; o.rowOffset.assign(querySlots.size() + 1, 0); o.rows.resize((size_t)std::max(capRows, 1)); o.ids.resize((size_t)std::max<int64_t>(capIds, 1));
    int nRows = 0; int64_t nIds = 0;
    check(corb_map_fusion_candidates_store(db, sub, querySlots.data(), queryEntries.data(), queryIds.data(), (int)querySlots.size(), global, entrySlot.data(), nnratio,
                                           checkOrientation ? 1 : 0, minMatches, o.rowOffset.data(), o.rows.data(), capRows, &nRows, o.ids.data(), capIds, &nIds),
          "corb_map_fusion_candidates_store");
    o.rows.resize((size_t)nRows); o.ids.resize((size_t)nIds);
    return o;
}

// ---- Tracking::TrackLocalMap on records (include/corb_track_local_map.h), mirrored as functions on the handles like the three above ----
// what the one call leaves: the lists as slots and ids, the matches into the list, mvbOutlier, and the result struct (ok = the reference's bool)
struct TrackLocalMapOutput { std::vector<int32_t> kfSlots, mpSlots, match; std::vector<uint64_t> mpIds; std::vector<uint8_t> outlier; CorbTrackLocalMapResult result; };
inline TrackLocalMapOutput TrackLocalMap(CorbCovis* graph, CorbKfStore* frames, int slot, const CorbTrackCamera& cam, const float* Tcw /* 16 */, const std::vector<int32_t>& prevKfSlots,
                                         const CorbTrackLocalMapParams& params, int maxKeyFrames, int maxMapPoints)
{
    TrackLocalMapOutput o; std::memset(&o.result, 0, sizeof(o.result));
    const int n = std::max(corb_kf_store_count(frames, slot), 0);
    o.kfSlots.resize((size_t)std::max(maxKeyFrames, 1)); o.mpSlots.resize((size_t)std::max(maxMapPoints, 1)); o.mpIds.resize((size_t)std::max(maxMapPoints, 1));
    o.match.assign((size_t)std::max(n, 1), -1); o.outlier.assign((size_t)std::max(n, 1), 0);
    check(corb_track_local_map(graph, frames, slot, &cam, Tcw, prevKfSlots.data(), (int)prevKfSlots.size(), &params, o.kfSlots.data(), maxKeyFrames, o.mpSlots.data(), o.mpIds.data(),
                               maxMapPoints, o.match.data(), o.outlier.data(), &o.result), "corb_track_local_map");
    o.kfSlots.resize((size_t)o.result.local.n_kf); o.mpSlots.resize((size_t)o.result.local.n_mp); o.mpIds.resize((size_t)o.result.local.n_mp);
    o.match.resize((size_t)n); o.outlier.resize((size_t)n);
    return o;
}
// the tail alone, after corb_track_pose_optimization(discard_outliers = 0): returns the reference's bool, *nMatchesInliers = mnMatchesInliers
inline bool TrackLocalMapStats(CorbKfStore* frames, int slot, CorbMpStore* map, int sensor, bool onlyTracking, uint64_t frameId, uint64_t lastRelocFrameId, int maxFrames, int* nMatchesInliers = nullptr)
{
    int32_t n = 0; int ok = 0;
    check(corb_track_local_map_stats(frames, slot, map, sensor, onlyTracking ? 1 : 0, frameId, lastRelocFrameId, maxFrames, &n, &ok), "corb_track_local_map_stats");
    if (nMatchesInliers) *nMatchesInliers = n;
    return ok != 0;
}

// ---- the initial pose of a tracked frame on records (include/corb_track_frame.h), mirrored as functions on the handles ----
// what either call leaves: the matches (the last frame's / the keyframe's feature per feature, or -1), the features the optimisation rejected, the result struct
struct TrackFrameOutput { std::vector<int32_t> match; std::vector<uint8_t> outlier; CorbTrackFrameResult result; };
// bool Tracking::TrackWithMotionModel() (Tracking.cc:886-949); Tlr = the last entry of mlRelativeFramePoses (16 floats), or nullptr: the last record's pose stands
inline TrackFrameOutput TrackWithMotionModel(CorbKfStore* frames, int curSlot, int lastSlot, CorbKfStore* kfs, int refSlot, CorbMpStore* map, const CorbTrackCamera& cam,
                                             const float* velocity /* 16 */, const float* Tlr, const CorbTrackFrameParams& params)
{
    TrackFrameOutput o; std::memset(&o.result, 0, sizeof(o.result));
    const int n = std::max(corb_kf_store_count(frames, curSlot), 0);
    o.match.assign((size_t)std::max(n, 1), -1); o.outlier.assign((size_t)std::max(n, 1), 0);
    check(corb_track_with_motion_model(frames, curSlot, lastSlot, kfs, refSlot, map, &cam, velocity, Tlr, &params, o.match.data(), o.outlier.data(), &o.result), "corb_track_with_motion_model");
    o.match.resize((size_t)n); o.outlier.resize((size_t)n);
    return o;
}
// bool Tracking::TrackReferenceKeyFrame() (Tracking.cc:775-817); voc = nullptr: the frame's record holds its FeatureVector already
inline TrackFrameOutput TrackReferenceKeyFrame(CorbKfStore* frames, int curSlot, int lastSlot, CorbKfStore* kfs, int refSlot, CorbMpStore* map, const CorbTrackCamera& cam,
                                               CorbVoc* voc, const CorbTrackFrameParams& params)
{
    TrackFrameOutput o; std::memset(&o.result, 0, sizeof(o.result));
    const int n = std::max(corb_kf_store_count(frames, curSlot), 0);
    o.match.assign((size_t)std::max(n, 1), -1); o.outlier.assign((size_t)std::max(n, 1), 0);
    check(corb_track_reference_keyframe(frames, curSlot, lastSlot, kfs, refSlot, map, &cam, voc, &params, o.match.data(), o.outlier.data(), &o.result), "corb_track_reference_keyframe");
    o.match.resize((size_t)n); o.outlier.resize((size_t)n);
    return o;
}
// the host's choice of Tracking.cc:301-316 (mState == OK, local mapping active): TrackReferenceKeyFrame when there is no velocity (velocity == nullptr) or the frame
// comes right after a relocalisation; otherwise TrackWithMotionModel, then TrackReferenceKeyFrame if it failed.  CheckReplacedInLastFrame (:304) runs once, in the
// first call made.  *usedMotionModel (optional) = the call whose result is returned was TrackWithMotionModel
inline TrackFrameOutput TrackInitialPose(CorbKfStore* frames, int curSlot, int lastSlot, CorbKfStore* kfs, int refSlot, CorbMpStore* map, const CorbTrackCamera& cam,
                                         const float* velocity, const float* Tlr, CorbVoc* voc, uint64_t frameId, uint64_t lastRelocFrameId, int sensor, bool* usedMotionModel = nullptr)
{
    CorbTrackFrameParams p; std::memset(&p, 0, sizeof(p));
    p.frame_id = frameId; p.sensor = sensor; p.only_tracking = 0; p.check_replaced = 1; p.check_orientation = 1;
    const bool reference_first = !velocity || frameId < lastRelocFrameId + 2;        // if(mVelocity.empty() || mCurrentFrame.mnId<mnLastRelocFrameId+2)
    if (usedMotionModel) *usedMotionModel = !reference_first;
    if (!reference_first) {
        p.nnratio = 0.9f; p.th = 0.f;
        TrackFrameOutput o = TrackWithMotionModel(frames, curSlot, lastSlot, kfs, refSlot, map, cam, velocity, Tlr, p);
        if (o.result.ok) return o;
        p.check_replaced = 0;
        if (usedMotionModel) *usedMotionModel = false;
    }
    p.nnratio = 0.7f; p.th = 0.f;
    return TrackReferenceKeyFrame(frames, curSlot, lastSlot, kfs, refSlot, map, cam, voc, p);
}
// the loops at the end of Tracking::Track: "Clean VO matches" (:438-447), asynchronous; then, after NeedNewKeyFrame / CreateNewKeyFrame, the outliers' points leave
// the frame (:463-467) and Tcr = mTcw * mpReferenceKF->GetPoseInverse() (:491) comes back: the next frame's Tlr
inline void CleanVOMatches(CorbKfStore* frames, int curSlot, CorbKfStore* kfs, int refSlot, CorbMpStore* map)
{
    check(corb_track_frame_finish(frames, curSlot, kfs, refSlot, map, 0, nullptr), "corb_track_frame_finish");
}
inline void TrackFrameFinish(CorbKfStore* frames, int curSlot, CorbKfStore* kfs, int refSlot, CorbMpStore* map, float* Tcr /* 16 */)
{
    check(corb_track_frame_finish(frames, curSlot, kfs, refSlot, map, 1, Tcr), "corb_track_frame_finish");
}

// ---- the camera trajectory (include/corb_trajectory.h): the log Tracking::Track appends, KeyFrame::mTcp, and System's three dumps under the reference's names ----
struct TrajectoryRows { int width = 0; std::vector<float> rows; std::vector<double> times; std::vector<int32_t> entry; std::vector<uint64_t> ids; CorbTrajStats stats{}; int n() const { return (int)times.size(); } };
class Trajectory {
    CorbTrajectory* h_ = nullptr; int capacity_, sensor_;
public:
    // sensor: System::eSensor (0 MONOCULAR, 1 STEREO, 2 RGBD): SaveTrajectoryTUM / KITTI refuse a monocular system (System.cc:256, :352)
    Trajectory(CorbCovis* graph, int capacityFrames, int sensor) : capacity_(capacityFrames), sensor_(sensor) { check(corb_traj_create(graph, capacityFrames, &h_), "corb_traj_create"); }
    ~Trajectory() { corb_traj_destroy(h_); }
    Trajectory(const Trajectory&) = delete;
    Trajectory& operator=(const Trajectory&) = delete;
    CorbTrajectory* handle() const { return h_; }
    void Reset() { check(corb_traj_reset(h_), "corb_traj_reset"); }
    // the end of Tracking::Track (:485-504): Tcr as TrackFrameFinish returned it, or nullptr: computed on the device from the two records
    void Append(CorbKfStore* frames, int curSlot, int refSlot, const float* Tcr, double timestamp, bool lost) { check(corb_traj_append(h_, frames, curSlot, refSlot, Tcr, timestamp, lost ? 1 : 0), "corb_traj_append"); }
    void AppendLost(bool lost = true) { check(corb_traj_append(h_, nullptr, -1, 0, nullptr, 0.0, lost ? 1 : 0), "corb_traj_append"); }       // the `else`: mlbLost.push_back(mState==LOST)
    void SetKeyFrameTime(int slot, double t) { check(corb_traj_set_keyframe_time(h_, slot, t), "corb_traj_set_keyframe_time"); }
    double KeyFrameTime(int slot) const { double t = 0; check(corb_traj_get_keyframe_time(h_, slot, &t), "corb_traj_get_keyframe_time"); return t; }
    // KeyFrame::SetBadFlag (:666), after corb_covis_reparent_children answered reference_sets_bad and before the caller sets CORB_KF_BAD
    void SetBadPose(int slot) { check(corb_traj_set_bad_pose(h_, slot), "corb_traj_set_bad_pose"); }
    void SetTcp(int slot, const float* Tcp) { check(corb_traj_set_tcp(h_, slot, Tcp), "corb_traj_set_tcp"); }
    void GetTcp(int slot, float* Tcp) const { check(corb_traj_get_tcp(h_, slot, Tcp), "corb_traj_get_tcp"); }
    std::vector<CorbTrajEntry> Entries() const
    {
        std::vector<CorbTrajEntry> e((size_t)capacity_); int n = 0;
        check(corb_traj_get_entries(h_, e.data(), capacity_, &n), "corb_traj_get_entries");
        e.resize((size_t)n);
        return e;
    }
    TrajectoryRows Frames(int format, int originSlot = -1) const
    {
        TrajectoryRows o; o.width = format == 0 ? 12 : 7;
        o.rows.resize((size_t)capacity_ * o.width); o.times.resize((size_t)capacity_); o.entry.resize((size_t)capacity_);
        int n = 0;
        check(corb_traj_frames(h_, originSlot, format, o.rows.data(), o.times.data(), o.entry.data(), capacity_, &n, &o.stats), "corb_traj_frames");
        o.rows.resize((size_t)n * o.width); o.times.resize((size_t)n); o.entry.resize((size_t)n);
        return o;
    }
    TrajectoryRows KeyFrames(int maxKeyFrames) const
    {
        TrajectoryRows o; o.width = 7;
        o.rows.resize((size_t)maxKeyFrames * 7); o.times.resize((size_t)maxKeyFrames); o.ids.resize((size_t)maxKeyFrames);
        int n = 0;
        check(corb_traj_keyframes(h_, o.rows.data(), o.times.data(), o.ids.data(), maxKeyFrames, &n), "corb_traj_keyframes");
        o.rows.resize((size_t)n * 7); o.times.resize((size_t)n); o.ids.resize((size_t)n);
        return o;
    }
    static std::string Format(int kind, const TrajectoryRows& r)
    {
        size_t len = 0;
        const int rc = corb_traj_format_rows(kind, r.rows.data(), r.times.data(), r.n(), nullptr, 0, &len);
        if (rc != CORB_ERR_CAPACITY) check(rc, "corb_traj_format_rows");
        std::string s(len, '\0');
        if (len) check(corb_traj_format_rows(kind, r.rows.data(), r.times.data(), r.n(), &s[0], len, &len), "corb_traj_format_rows");
        return s;
    }
    // false: "ERROR: SaveTrajectoryTUM cannot be used for monocular." -- nothing is written
    bool SaveTrajectoryTUM(const std::string& filename, int originSlot = -1) { if (sensor_ == 0) return false; check(corb_traj_save(h_, originSlot, 1, filename.c_str()), "corb_traj_save"); return true; }
    bool SaveTrajectoryKITTI(const std::string& filename, int originSlot = -1) { if (sensor_ == 0) return false; check(corb_traj_save(h_, originSlot, 0, filename.c_str()), "corb_traj_save"); return true; }
    void SaveKeyFrameTrajectoryTUM(const std::string& filename) { check(corb_traj_save(h_, -1, 2, filename.c_str()), "corb_traj_save"); }
};

// ---- LoopClosing::DetectLoop on records (include/corb_loop_detect.h): a plain mirror over the C calls ----
// one keyframe's DetectLoop: the outcome and counts, vpCandidateKFs as database entries and store slots, mvpEnoughConsistentCandidates as positions in them
struct LoopDetection { CorbLoopDetectResult result{}; std::vector<int32_t> candEntries, candSlots, enough; bool detected() const { return result.outcome == CORB_LOOP_DETECTED; } };
struct ConsistentGroups { std::vector<int32_t> counters, offsets, members; int n() const { return (int)counters.size(); } };
class LoopDetector {
    CorbLoopDetector* h_ = nullptr; int maxCandidates_, maxGroups_;
    LoopDetection take(const CorbLoopDetectResult& r, const int32_t* ce, const int32_t* cs, const int32_t* en) const
    {
        LoopDetection d; d.result = r;
        const int nc = std::min(std::max(r.n_candidates, 0), maxCandidates_), ne = std::min(std::max(r.n_enough, 0), maxCandidates_);
        d.candEntries.assign(ce, ce + nc); d.candSlots.assign(cs, cs + nc); d.enough.assign(en, en + ne);
        return d;
    }
public:
    LoopDetector(CorbCovis* graph, CorbKfDb* db, int maxCandidates, int maxGroups) : maxCandidates_(maxCandidates), maxGroups_(maxGroups)
    {
        check_abi();
        check(corb_loop_detector_create(graph, db, maxCandidates, maxGroups, &h_), "corb_loop_detector_create");
    }
    ~LoopDetector() { corb_loop_detector_destroy(h_); }
    LoopDetector(const LoopDetector&) = delete;
    LoopDetector& operator=(const LoopDetector&) = delete;
    CorbLoopDetector* handle() const { return h_; }
    int maxCandidates() const { return maxCandidates_; }
    void Bind(const std::vector<int32_t>& slots, const std::vector<int32_t>& entries)
    {
        if (slots.size() != entries.size()) throw std::invalid_argument("LoopDetector::Bind: slots and entries differ in length");
        check(corb_loop_detector_bind(h_, slots.data(), entries.data(), (int)slots.size()), "corb_loop_detector_bind");
    }
    void SetLastLoop(uint64_t id) { check(corb_loop_detector_set_last_loop(h_, id), "corb_loop_detector_set_last_loop"); }       // mLastLoopKFid = mpCurrentKF->mnId (:591)
    uint64_t LastLoop() const { uint64_t id = 0; check(corb_loop_detector_get_last_loop(h_, &id), "corb_loop_detector_get_last_loop"); return id; }
    void Reset() { check(corb_loop_detector_reset(h_), "corb_loop_detector_reset"); }                                            // :647
    void ClearGroups() { check(corb_loop_detector_clear_groups(h_), "corb_loop_detector_clear_groups"); }
    void DropSlot(int slot) { check(corb_loop_detector_drop_slot(h_, slot), "corb_loop_detector_drop_slot"); }
    ConsistentGroups Groups(int maxSlots) const
    {
        ConsistentGroups g; g.counters.resize((size_t)maxGroups_); g.offsets.resize((size_t)maxGroups_ + 1); g.members.resize((size_t)maxGroups_ * (size_t)std::max(maxSlots, 1));
        int ng = 0, nm = 0;
        check(corb_loop_detector_get_groups(h_, g.counters.data(), g.offsets.data(), g.members.data(), maxGroups_, (int)g.members.size(), &ng, &nm), "corb_loop_detector_get_groups");
        g.counters.resize((size_t)ng); g.offsets.resize((size_t)ng + 1); g.members.resize((size_t)nm);
        return g;
    }
    // bool LoopClosing::DetectLoop() for mpCurrentKF = the record in `slot`
    LoopDetection DetectLoop(int slot)
    {
        const size_t mc = (size_t)maxCandidates_;
        std::vector<int32_t> ce(mc), cs(mc), en(mc); CorbLoopDetectResult r; std::memset(&r, 0, sizeof(r));
        check(corb_loop_detect(h_, slot, &r, ce.data(), cs.data(), en.data()), "corb_loop_detect");
        return take(r, ce.data(), cs.data(), en.data());
    }
    // DetectLoop for the queue in order, up to and with the first detection: one entry per consumed keyframe
    std::vector<LoopDetection> DetectLoopQueue(const std::vector<int32_t>& slots)
    {
        const size_t n = slots.size(), mc = (size_t)maxCandidates_;
        std::vector<CorbLoopDetectResult> r(std::max(n, (size_t)1)); std::vector<int32_t> ce(std::max(n, (size_t)1) * mc), cs(ce.size()), en(ce.size());
        std::memset(r.data(), 0, r.size() * sizeof(CorbLoopDetectResult));
        int done = 0;
        check(corb_loop_detect_queue(h_, slots.data(), (int)n, r.data(), ce.data(), cs.data(), en.data(), &done), "corb_loop_detect_queue");
        std::vector<LoopDetection> out;
        for (int k = 0; k < done; k++) out.push_back(take(r[(size_t)k], ce.data() + (size_t)k * mc, cs.data() + (size_t)k * mc, en.data() + (size_t)k * mc));
        return out;
    }
};
}  // namespace corb
