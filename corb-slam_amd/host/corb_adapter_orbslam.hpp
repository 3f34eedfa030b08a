// corb_adapter_orbslam.hpp -- the reference's ORBmatcher / Optimizer SIGNATURES on top of corb_host.hpp.
//
//   int  ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)                        corbslam_client/include/ORBmatcher.h:57
//   int  ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)                     :58
//   int  ORBmatcher::SearchByBoWInServer(KeyFrame*, KeyFrame*, vector<MapPoint*>&)             :60
//   int  ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12, vector<pair<size_t,size_t>>&, bool)   :66-67
//   int  ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>&, int th)  :52-53 (loop closing / map fusion)
//   int  ORBmatcher::SearchForInitialization(Frame&, Frame&, vector<cv::Point2f>&, vector<int>&, int windowSize)         :62-63 (monocular initialisation)
//   void Optimizer::BundleAdjustment(const vector<KeyFrame*>&, const vector<MapPoint*>&, int, bool*, unsigned long, bool)   include/Optimizer.h:42-44
//   void Optimizer::GlobalBundleAdjustemnt(Cache*, int, bool*, unsigned long, bool)            :45-46
//   int  Optimizer::PoseOptimization(Frame*)                                                   :51
//   Sim3Solver(KeyFrame*, KeyFrame*, const vector<MapPoint*>&, bool) / SetRansacParameters / iterate / find / GetEstimated*   include/Sim3Solver.h:39-49
//   Initializer(const Frame&, float sigma, int iterations) / Initialize(const Frame&, const vector<int>&, cv::Mat&, cv::Mat&, vector<cv::Point3f>&, vector<bool>&)   include/Initializer.h:38-43
//
// The adapters FLATTEN the reference's pointer graph into the arrays of the C-ABI (KeyFrame* / Frame& -> descriptors, keypoints, mvuRight,
// "has a good MapPoint" flags, DBoW2::FeatureVector; Cache* -> poses, per-keyframe intrinsics, points, observations), call the accelerator,
// and MAP the indices BACK (match index -> MapPoint*, estimates -> SetPose / SetWorldPos or mTcwGBA / mPosGBA by the nLoopKF policy of
// Optimizer.cc:216-262).  They are templates over the reference's class types and touch them only through the member names the reference
// itself uses at the cited lines, so that
//   * on a tree with the reference's headers (OpenCV, Boost, ROS present) the aliases at the bottom of this file instantiate them with
//     ORB_SLAM2::KeyFrame / Frame / MapPoint / Cache and cv::Mat -- a drop-in for ORBmatcher.cc / Optimizer.cc on this path;
//   * in this repository (none of those dependencies exist) the SAME template code is compiled and run against small test doubles that carry
//     those member names (tests/host/mock_orbslam.hpp, driven by tests/host/adapter_main.cpp on the GPU box) and its outputs are compared
//     with the oracle (tests/test_gpu_host.py).
#pragma once
#include "corb_host.hpp"
#include <corb_voc_train.h>
#include <corb_keyframe_insert.h>
#include <corb_map_publish.h>
#include <corb_essential_graph.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <list>
#include <map>
#include <set>
#include <thread>
#include <utility>
#include <vector>
#include <cmath>
#include <type_traits>

namespace corb {
namespace adapt {

// ---- the only operations used on the reference's matrix / keypoint types ----
template <class Mat> inline float matf(const Mat& m, int r, int c) { return m.template at<float>(r, c); }
template <class Mat> inline float matf(const Mat& m, int i) { return m.template at<float>(i); }
template <class Mat> inline const uint8_t* desc_row(const Mat& m, int r) { return m.template ptr<uint8_t>(r); }            // cv::Mat::ptr<uchar>(row)
template <class Mat> struct MatFactory;              // MatFactory<Mat>::from_floats(rows, cols, const float*) -> an owning CV_32F matrix
template <class KP> inline CorbKeyPoint to_kp(const KP& k)
{ CorbKeyPoint o; o.x = k.pt.x; o.y = k.pt.y; o.size = k.size; o.angle = k.angle; o.response = k.response; o.octave = k.octave; o.class_id = k.class_id; return o; }

// DBoW2::FeatureVector = std::map<NodeId, std::vector<unsigned int>>: ascending node ids, as the merge-walk of the matchers needs them
template <class FV> inline FeatureVector flatten_featvec(const FV& fv)
{ FeatureVector o; for (auto it = fv.begin(); it != fv.end(); ++it) o.add((uint32_t)it->first, it->second); return o; }

// What SearchByBoW / SearchForTriangulation read from a KeyFrame: mDescriptors, mvKeysUn, mvuRight, GetMapPointMatches(), mFeatVec.
// good_only: vpMapPoints[i] && !isBad() (BoW matchers, ORBmatcher.cc:194-199, 693-699); otherwise any non-NULL entry (GetMapPoint(idx) != NULL,
// SearchForTriangulation :835-838, :858-862)
template <class KeyFrame> FeatureSet flatten_keyframe(KeyFrame* pKF, bool good_only, bool angle_from_mvKeys = false)
{
    FeatureSet s; const int N = pKF->N;
    s.desc.data.resize((size_t)N * 32); s.keysUn.resize(N); s.uRight.resize(N); s.hasGoodMapPoint.assign(N, 0);
    const auto vpMP = pKF->GetMapPointMatches();
    for (int i = 0; i < N; i++) {
        std::memcpy(&s.desc.data[(size_t)i * 32], desc_row(pKF->mDescriptors, i), 32);
        s.keysUn[i] = to_kp(pKF->mvKeysUn[i]);
        if (angle_from_mvKeys) s.keysUn[i].angle = pKF->mvKeys[i].angle;       // the "frame" side of SearchByBoWInServer reads F->mvKeys[..].angle (:375)
        s.uRight[i] = pKF->mvuRight[i];
        auto* pMP = i < (int)vpMP.size() ? vpMP[i] : nullptr;
        s.hasGoodMapPoint[i] = pMP && (!good_only || !pMP->isBad()) ? 1 : 0;
    }
    s.featVec = flatten_featvec(pKF->mFeatVec);
    return s;
}
// The Frame side of SearchByBoW(KeyFrame*, Frame&): mDescriptors, mFeatVec and F.mvKeys[..].angle (ORBmatcher.cc:241)
template <class Frame> FeatureSet flatten_frame(Frame& F)
{
    FeatureSet s; const int N = F.N;
    s.desc.data.resize((size_t)N * 32); s.keysUn.resize(N); s.uRight.resize(N); s.hasGoodMapPoint.assign(N, 1);
    for (int i = 0; i < N; i++) {
        std::memcpy(&s.desc.data[(size_t)i * 32], desc_row(F.mDescriptors, i), 32);
        s.keysUn[i] = to_kp(F.mvKeysUn[i]); s.keysUn[i].angle = F.mvKeys[i].angle;
        s.uRight[i] = F.mvuRight[i];
    }
    s.featVec = flatten_featvec(F.mFeatVec);
    return s;
}

template <class KeyFrame, class Frame, class MapPoint, class Mat>
class ORBmatcherT {
public:
    static constexpr int TH_LOW = corb::ORBmatcher::TH_LOW, TH_HIGH = corb::ORBmatcher::TH_HIGH, HISTO_LENGTH = corb::ORBmatcher::HISTO_LENGTH;
    ORBmatcherT(float nnratio = 0.6f, bool checkOri = true, int device = 0) : m_(nnratio, checkOri, device) {}

    static int DescriptorDistance(const Mat& a, const Mat& b) { return corb::ORBmatcher::DescriptorDistance(desc_row(a, 0), desc_row(b, 0)); }

    // ORBmatcher.cc:162-291
    int SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches)
    {
        const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
        vpMapPointMatches = std::vector<MapPoint*>(F.N, static_cast<MapPoint*>(nullptr));
        std::vector<int32_t> m;
        const int n = m_.SearchByBoW(flatten_keyframe(pKF, true), flatten_frame(F), m);
        for (int iF = 0; iF < F.N; iF++) if (m[iF] >= 0) vpMapPointMatches[iF] = vpMapPointsKF[m[iF]];
        return n;
    }
    // ORBmatcher.cc:294-423 (server-side map fusion: the "frame" is a KeyFrame of the other map)
    int SearchByBoWInServer(KeyFrame* pKF, KeyFrame* F, std::vector<MapPoint*>& vpMapPointMatches)
    {
        const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
        vpMapPointMatches = std::vector<MapPoint*>(F->N, static_cast<MapPoint*>(nullptr));
        FeatureSet fs = flatten_keyframe(F, true, true); std::fill(fs.hasGoodMapPoint.begin(), fs.hasGoodMapPoint.end(), 1);
        std::vector<int32_t> m;
        const int n = m_.SearchByBoWInServer(flatten_keyframe(pKF, true), fs, m);
        for (int iF = 0; iF < F->N; iF++) if (m[iF] >= 0) vpMapPointMatches[iF] = vpMapPointsKF[m[iF]];
        return n;
    }
    // ORBmatcher.cc:657-790 (loop closing / Sim3): vpMatches12[i1] = the MapPoint of the matched feature of pKF2
    int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12)
    {
        const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
        vpMatches12 = std::vector<MapPoint*>(vpMapPoints1.size(), static_cast<MapPoint*>(nullptr));
        std::vector<int32_t> m;
        const int n = m_.SearchByBoW_KF(flatten_keyframe(pKF1, true), flatten_keyframe(pKF2, true), m);
        for (size_t i1 = 0; i1 < vpMatches12.size() && i1 < m.size(); i1++) if (m[i1] >= 0) vpMatches12[i1] = vpMapPoints2[m[i1]];
        return n;
    }
    // ORBmatcher.cc:792-958.  The epipole (:799-808): C2 = R2w*Cw + t2w in float matrices (cv::gemm accumulates a float product in double)
    int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, Mat F12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs, const bool bOnlyStereo)
    {
        const Mat Cw = pKF1->GetCameraCenter(), R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
        float C2[3];
        for (int i = 0; i < 3; i++) {
            double acc = 0; for (int k = 0; k < 3; k++) acc += (double)matf(R2w, i, k) * (double)matf(Cw, k);
            C2[i] = (float)acc + matf(t2w, i);
        }
        const float invz = 1.0f / C2[2];
        const float ex = pKF2->fx * C2[0] * invz + pKF2->cx, ey = pKF2->fy * C2[1] * invz + pKF2->cy;
        float F[9]; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) F[3 * i + j] = matf(F12, i, j);
        return m_.SearchForTriangulation(flatten_keyframe(pKF1, false), flatten_keyframe(pKF2, false), F, ex, ey, pKF2->mvScaleFactors, pKF2->mvLevelSigma2,
                                         vMatchedPairs, bOnlyStereo);
    }
    // LocalMapping::CreateNewMapPoints' "Triangulate each match" loop (C/src/LocalMapping.cc:262-398) for the pairs SearchForTriangulation returned for ONE neighbour:
    // both keyframes are flattened (mvKeysUn, mvuRight, mvDepth, GetPose(), fx .. mbf, mb, mvScaleFactors), the pairs go through corb_triangulate_pairs, and the accepted
    // ones come back as (idx1, idx2, x3D) for the caller's `new MapPoint(x3D, mpCurrentKeyFrame, mpCacher)` + AddObservation / AddMapPoint (:401-415) -- which it does
    // before matching the next neighbour, as the reference does.  Returns their number.
    struct NewPoint { size_t idx1, idx2; float x3D[3]; };
    static int CreateNewMapPoints(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<std::pair<size_t, size_t>>& vMatchedIndices, std::vector<NewPoint>& vNew, int device = 0)
    {
        vNew.clear();
        const int n = (int)vMatchedIndices.size();
        if (n == 0) return 0;
        std::vector<CorbKeyPoint> kp[2]; CorbNewPointSide side[2]; KeyFrame* kfs[2] = {pKF1, pKF2};
        for (int s = 0; s < 2; s++) {
            KeyFrame* pKF = kfs[s];
            kp[s].reserve(pKF->mvKeysUn.size());
            for (const auto& k : pKF->mvKeysUn) kp[s].push_back(to_kp(k));
            const Mat T = pKF->GetPose();
            CorbNewPointSide& d = side[s];
            d.keys_un = kp[s].data(); d.u_right = pKF->mvuRight.data(); d.depth = pKF->mvDepth.data(); d.n = (int)kp[s].size();
            for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) d.Tcw[4 * i + j] = matf(T, i, j);
            d.fx = pKF->fx; d.fy = pKF->fy; d.cx = pKF->cx; d.cy = pKF->cy; d.bf = pKF->mbf; d.mb = pKF->mb;
            d.scale = pKF->mvScaleFactors.data(); d.nlevels = (int)pKF->mvScaleFactors.size();
        }
        std::vector<int32_t> pairs(2 * (size_t)n); std::vector<float> x3d(3 * (size_t)n); std::vector<uint8_t> status((size_t)n), source((size_t)n);
        for (int i = 0; i < n; i++) { pairs[2 * (size_t)i] = (int32_t)vMatchedIndices[i].first; pairs[2 * (size_t)i + 1] = (int32_t)vMatchedIndices[i].second; }
        int nnew = 0;
        check(corb_triangulate_pairs(&side[0], &side[1], pairs.data(), n, x3d.data(), status.data(), source.data(), &nnew, device), "corb_triangulate_pairs");
        for (int i = 0; i < n; i++)
            if (status[i] == CORB_NP_OK) vNew.push_back(NewPoint{vMatchedIndices[i].first, vMatchedIndices[i].second, {x3d[3 * (size_t)i], x3d[3 * (size_t)i + 1], x3d[3 * (size_t)i + 2]}});
        return nnew;
    }
    // ORBmatcher.cc:425-538 -- LoopClosing::ComputeSim3 (C/src/LoopClosing.cc:377) and the server's map fusion (S/src/GlobalOptimize.cpp:199) call it with the loop
    // keyframe's covisible points right before CorrectLoop / the global BA.  What the reference reads: pKF->fx.., mnMinX.., mvScaleFactors, mfLogScaleFactor, mvKeysUn,
    // mDescriptors (GetFeaturesInArea + the loop body); pMP->isBad / GetWorldPos / GetNormal / Get{Min,Max}DistanceInvariance / PredictScale / GetDescriptor.  The two
    // raw distances are read through GetMinDistance() / GetMaxDistance() (the accessors MapPoint.h gains), the getters' 0.8f / 1.2f are applied on the device.
    int SearchByProjection(KeyFrame* pKF, Mat Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th)
    {
        const int N = pKF->N;
        std::vector<CorbKeyPoint> keys(N); std::vector<uint8_t> desc((size_t)N * 32), hasMatch(N, 0);
        for (int i = 0; i < N; i++) { keys[i] = to_kp(pKF->mvKeysUn[i]); std::memcpy(&desc[(size_t)i * 32], desc_row(pKF->mDescriptors, i), 32); hasMatch[i] = (i < (int)vpMatched.size() && vpMatched[i]) ? 1 : 0; }
        CorbKeyFrameView K; std::memset(&K, 0, sizeof(K));
        K.keys_un = keys.data(); K.u_right = pKF->mvuRight.data(); K.desc = desc.data(); K.n = N;
        K.min_x = (float)pKF->mnMinX; K.min_y = (float)pKF->mnMinY; K.max_x = (float)pKF->mnMaxX; K.max_y = (float)pKF->mnMaxY;
        K.scale = pKF->mvScaleFactors.data(); K.inv_level_sigma2 = pKF->mvInvLevelSigma2.data(); K.nlevels = (int32_t)pKF->mvScaleFactors.size();
        K.log_scale_factor = pKF->mfLogScaleFactor; K.fx = pKF->fx; K.fy = pKF->fy; K.cx = pKF->cx; K.cy = pKF->cy; K.bf = pKF->mbf;
        std::set<MapPoint*> spAlreadyFound(vpMatched.begin(), vpMatched.end());       // :441-442
        spAlreadyFound.erase(static_cast<MapPoint*>(nullptr));
        std::vector<CorbMapPointView> pts(vpPoints.size()); std::vector<uint8_t> pdesc(vpPoints.size() * 32 + 32, 0);
        for (size_t i = 0; i < vpPoints.size(); i++) {
            MapPoint* pMP = vpPoints[i]; CorbMapPointView& v = pts[i]; std::memset(&v, 0, sizeof(v));
            if (!pMP || pMP->isBad() || spAlreadyFound.count(pMP)) continue;          // :452 (valid stays 0)
            const Mat X = pMP->GetWorldPos(), Nn = pMP->GetNormal(), D = pMP->GetDescriptor();
            for (int a = 0; a < 3; a++) { v.world[a] = matf(X, a); v.normal[a] = matf(Nn, a); }
            v.min_distance = pMP->GetMinDistance(); v.max_distance = pMP->GetMaxDistance(); v.valid = 1;
            std::memcpy(&pdesc[i * 32], desc_row(D, 0), 32);
        }
        float S[16]; for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) S[4 * r + c] = matf(Scw, r, c);
        std::vector<int32_t> m;
        const int n = m_.SearchByProjection(K, hasMatch, S, pts, pdesc.data(), th, m);
        if ((int)vpMatched.size() < N) vpMatched.resize(N, static_cast<MapPoint*>(nullptr));
        for (int idx = 0; idx < N; idx++) if (m[idx] >= 0) vpMatched[idx] = vpPoints[m[idx]];      // :530
        return n;
    }
    // ORBmatcher.cc:540-655 (Tracking::MonocularInitialization, C/src/Tracking.cc:606).  Point2f = cv::Point2f (anything with float x, y).  What the reference reads:
    // F1.mvKeysUn (octave, angle), F1.mDescriptors, F2.GetFeaturesInArea (mvKeysUn, the grid over mnMinX .. mnMaxY), F2.mDescriptors, F2.mvKeysUn[..].angle / .pt
    template <class Point2f>
    int SearchForInitialization(Frame& F1, Frame& F2, std::vector<Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize = 10)
    {
        auto view = [](Frame& F, std::vector<CorbKeyPoint>& k, std::vector<uint8_t>& d) {
            k.resize(F.N); d.resize((size_t)F.N * 32);
            for (int i = 0; i < F.N; i++) { k[i] = to_kp(F.mvKeysUn[i]); std::memcpy(&d[(size_t)i * 32], desc_row(F.mDescriptors, i), 32); }
            CorbFrameView v; std::memset(&v, 0, sizeof(v));
            v.keys_un = k.data(); v.desc = d.data(); v.n = F.N; v.min_x = Frame::mnMinX; v.min_y = Frame::mnMinY; v.max_x = Frame::mnMaxX; v.max_y = Frame::mnMaxY;
            return v;
        };
        std::vector<CorbKeyPoint> k1, k2; std::vector<uint8_t> d1, d2;
        const CorbFrameView v1 = view(F1, k1, d1), v2 = view(F2, k2, d2);
        std::vector<float> pm((size_t)2 * F1.N);
        for (int i = 0; i < F1.N; i++) { pm[2 * i] = vbPrevMatched[i].x; pm[2 * i + 1] = vbPrevMatched[i].y; }
        std::vector<int32_t> m;
        const int n = m_.SearchForInitialization(v1, v2, pm, m, windowSize);
        vnMatches12 = std::vector<int>(F1.N, -1);                                   // :543
        for (int i = 0; i < F1.N; i++) { vnMatches12[i] = m[i]; if (m[i] >= 0) { vbPrevMatched[i].x = pm[2 * i]; vbPrevMatched[i].y = pm[2 * i + 1]; } }      // :650-653
        return n;
    }
private:
    corb::ORBmatcher m_;
};

// ---- Converter::toSE3Quat -> SE3Quat -> Converter::toCvMat round trip of a float pose (what the reference writes back for a keyframe whose vertex
// was fixed by id only: mnId == 1 is fixed in the graph but not skipped by the write-back loop, Optimizer.cc:94, 222) ----
inline void se3_roundtrip(const float* T, float* out)
{
    const double R[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };
    double q[4]; double t = R[0] + R[4] + R[8];
    if (t > 0) { t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t; q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t; }
    else {
        int i = 0; if (R[4] > R[0]) i = 1; if (R[8] > R[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t; q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t; q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    }
    if (q[3] < 0) for (double& v : q) v = -v;
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (double& v : q) v /= n;
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2], twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    const double Ro[9] = { 1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy) };
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) out[4 * r + c] = (float)Ro[3 * r + c]; out[4 * r + 3] = T[4 * r + 3]; }
    out[12] = out[13] = out[14] = 0; out[15] = 1;
}

// bool* pbStopFlag (the reference's type, polled by g2o between LM trials) -> the C-ABI's volatile int*: a watcher copies it while the call runs
struct StopBridge {
    volatile int flag = 0; std::atomic<bool> done{false}; std::thread th;
    explicit StopBridge(bool* pb) { if (pb) { flag = *pb ? 1 : 0; th = std::thread([this, pb] { while (!done.load()) { if (*pb) flag = 1; std::this_thread::sleep_for(std::chrono::microseconds(200)); } }); } }
    ~StopBridge() { done.store(true); if (th.joinable()) th.join(); }
    volatile int* ptr(bool* pb) { return pb ? &flag : nullptr; }
};

template <class KeyFrame, class Frame, class MapPoint, class Cache, class Mat>
class OptimizerT {
public:
    // Optimizer.cc:43-51
    static void GlobalBundleAdjustemnt(Cache* pCache, int nIterations = 5, bool* pbStopFlag = nullptr, const unsigned long nLoopKF = 0, const bool bRobust = true, int device = 0)
    {
        std::vector<KeyFrame*> vpKFs = pCache->getAllKeyFramesInMap();
        std::vector<MapPoint*> vpMP = pCache->GetAllMapPointsFromMap();
        BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust, device);
    }

    // Optimizer.cc:54-270.  Graph build :84-203 (vertex ids = mnId, so the solver's ordering is ascending mnId: the arrays are sorted that way);
    // write-back :216-262.
    static void BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag,
                                 const unsigned long nLoopKF, const bool bRobust, int device = 0)
    {
        unsigned long maxKFid = 0;
        std::vector<KeyFrame*> kfs;                                       // non-bad keyframes, ascending mnId
        for (KeyFrame* pKF : vpKFs) { if (pKF && pKF->mnId > maxKFid) maxKFid = pKF->mnId; if (pKF->isBad()) continue; kfs.push_back(pKF); }
        std::sort(kfs.begin(), kfs.end(), [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; });
        kfs.erase(std::unique(kfs.begin(), kfs.end()), kfs.end());
        std::map<KeyFrame*, int> kfIndex; for (size_t i = 0; i < kfs.size(); i++) kfIndex[kfs[i]] = (int)i;
        corb::Optimizer::Graph g;
        g.Tcw.resize(16 * kfs.size()); g.kfFixed.resize(kfs.size()); g.intr.resize(5 * kfs.size());
        for (size_t i = 0; i < kfs.size(); i++) {
            KeyFrame* pKF = kfs[i];
            const Mat T = pKF->GetPose();
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) g.Tcw[16 * i + 4 * r + c] = matf(T, r, c);
            g.kfFixed[i] = (pKF->mnId == 1 || pKF->getFixed()) ? 1 : 0;       // :94
            float* in = &g.intr[5 * i]; in[0] = pKF->fx; in[1] = pKF->fy; in[2] = pKF->cx; in[3] = pKF->cy; in[4] = pKF->mbf;   // e->fx = pKF->fx ... e->bf = pKF->mbf (:160-163, :189-193)
        }
        if (!kfs.empty()) { g.fx = kfs[0]->fx; g.fy = kfs[0]->fy; g.cx = kfs[0]->cx; g.cy = kfs[0]->cy; g.bf = kfs[0]->mbf; }
        std::vector<MapPoint*> mps;                                       // non-bad map points, ascending mnId
        for (MapPoint* pMP : vpMP) if (pMP && !pMP->isBad()) mps.push_back(pMP);
        std::sort(mps.begin(), mps.end(), [](MapPoint* a, MapPoint* b) { return a->mnId < b->mnId; });
        mps.erase(std::unique(mps.begin(), mps.end()), mps.end());
        std::vector<int> nEdges(mps.size(), 0);
        g.worldPos.resize(3 * mps.size()); g.mpFixed.resize(mps.size());
        for (size_t m = 0; m < mps.size(); m++) {
            MapPoint* pMP = mps[m];
            const Mat X = pMP->GetWorldPos();
            for (int a = 0; a < 3; a++) g.worldPos[3 * m + a] = matf(X, a);
            g.mpFixed[m] = pMP->getFixed() ? 1 : 0;                       // :120
            const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
            for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
                KeyFrame* pKF = mit->first;
                if (pKF->isBad() || pKF->mnId > maxKFid) continue;        // :131-132
                auto it = kfIndex.find(pKF); if (it == kfIndex.end()) continue;   // :134-135 (allKFId)
                nEdges[m]++;
                const auto& kpUn = pKF->mvKeysUn[mit->second];
                CorbBAEdge e; e.pose = it->second; e.point = (int32_t)m; e.u = kpUn.pt.x; e.v = kpUn.pt.y;
                e.u_right = pKF->mvuRight[mit->second];                   // < 0: EdgeSE3ProjectXYZ, else EdgeStereoSE3ProjectXYZ (:141, :166)
                e.inv_sigma2 = pKF->mvInvLevelSigma2[kpUn.octave];
                g.observations.push_back(e);
            }
        }
        std::vector<float> Tout, Xout;
        {
            StopBridge stop(pbStopFlag);
            corb::Optimizer::BundleAdjustment(g, Tout, Xout, nIterations, stop.ptr(pbStopFlag), bRobust, device);
        }
        // Keyframes (:216-237): every non-bad keyframe that is not getFixed() -- including mnId == 1, whose estimate did not move
        for (size_t i = 0; i < kfs.size(); i++) {
            KeyFrame* pKF = kfs[i];
            if (pKF->getFixed()) continue;
            float T[16];
            if (g.kfFixed[i]) se3_roundtrip(&g.Tcw[16 * i], T); else std::memcpy(T, &Tout[16 * i], sizeof(T));
            if (nLoopKF == 0) { pKF->SetPose(MatFactory<Mat>::from_floats(4, 4, T)); pKF->mpCacher->addUpdateKeyframe(pKF); }
            else { pKF->mTcwGBA = MatFactory<Mat>::from_floats(4, 4, T); pKF->mnBAGlobalForKF = nLoopKF; }
        }
        // Points (:240-262): those that got at least one edge (vbNotIncludedMP) and are not getFixed()
        for (size_t m = 0; m < mps.size(); m++) {
            MapPoint* pMP = mps[m];
            if (nEdges[m] == 0 || pMP->getFixed()) continue;
            if (nLoopKF == 0) { pMP->SetWorldPos(MatFactory<Mat>::from_floats(3, 1, &Xout[3 * m])); pMP->getCache()->addUpdateMapPoint(pMP); pMP->UpdateNormalAndDepth(); }
            else { pMP->mPosGBA = MatFactory<Mat>::from_floats(3, 1, &Xout[3 * m]); pMP->mnBAGlobalForKF = nLoopKF; }
        }
    }

    // Optimizer.cc:272-485
    static int PoseOptimization(Frame* pFrame, int device = 0)
    {
        corb::Optimizer::FrameObservations f;
        f.fx = pFrame->fx; f.fy = pFrame->fy; f.cx = pFrame->cx; f.cy = pFrame->cy; f.bf = pFrame->mbf;
        std::vector<size_t> vnIndexEdge;
        const int N = pFrame->N;
        for (int i = 0; i < N; i++) {
            MapPoint* pMP = pFrame->mvpMapPoints[i].getMapPoint();        // (CORB-SLAM keeps LightMapPoint handles in the Frame, :314)
            if (!pMP) continue;
            pFrame->mvbOutlier[i] = false;                                // :321, :352
            const auto& kpUn = pFrame->mvKeysUn[i];
            const Mat Xw = pMP->GetWorldPos();
            for (int a = 0; a < 3; a++) f.worldPos.push_back(matf(Xw, a));
            f.u.push_back(kpUn.pt.x); f.v.push_back(kpUn.pt.y); f.uRight.push_back(pFrame->mvuRight[i]);
            f.invSigma2.push_back(pFrame->mvInvLevelSigma2[kpUn.octave]);
            vnIndexEdge.push_back((size_t)i);
        }
        const int nInitialCorrespondences = (int)vnIndexEdge.size();
        if (nInitialCorrespondences < 3) return 0;                        // :396-397
        float Tcw[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw[4 * r + c] = matf(pFrame->mTcw, r, c);
        std::vector<uint8_t> outl;
        const int nGood = corb::Optimizer::PoseOptimization(Tcw, f, outl, device);
        for (size_t k = 0; k < vnIndexEdge.size(); k++) pFrame->mvbOutlier[vnIndexEdge[k]] = outl[k] != 0;
        pFrame->SetPose(MatFactory<Mat>::from_floats(4, 4, Tcw));        // :480-482
        return nGood;
    }
};

// ---- KeyFrame / MapPoint objects <-> device-resident store records (what the reference moves as boost text archives) ----
// The client side of Cache::runUpdateToServer (C/src/Cache.cc:322-375) files its new keyframes and map points in the stores and calls corb_map_push_ex;
// the server side of MapFusion::insertKeyFrameToMap / insertMapPointToMap (S/src/MapFusion.cpp:31-190) finds them in its own stores at the destination
// slots, re-bases them (corb_rebase_map_store) and runs the fused global BA on the records (corb_ba_solve_store); ReadBack* applies what the
// records hold to the objects with the policy of Optimizer.cc:216-262 (nLoopKF == 0: SetPose / SetWorldPos + cache marks; else mTcwGBA / mPosGBA).
template <class KeyFrame, class MapPoint, class Mat>
class MapStoreT {
public:
    // the record of one keyframe: mvKeysUn (the keypoints the optimiser and the matchers read; rectified stereo: = mvKeys), mDescriptors, mvuRight, mvDepth,
    // mFeatVec, mvpMapPoints as ids, and the header fields of KeyFrame.h:65-79
    static void PutKeyFrame(CorbKfStore* store, int slot, KeyFrame* pKF, int clientId = 0)
    {
        const int N = pKF->N;
        std::vector<CorbKeyPoint> kp(N); std::vector<uint8_t> desc((size_t)N * 32); std::vector<float> depth(N, -1.f); std::vector<uint64_t> ids(N, CORB_NO_MAP_POINT);
        const auto vpMP = pKF->GetMapPointMatches();
        for (int i = 0; i < N; i++) {
            kp[i] = to_kp(pKF->mvKeysUn[i]);
            if (!pKF->mDescriptors.empty()) std::memcpy(&desc[(size_t)i * 32], desc_row(pKF->mDescriptors, i), 32);
            auto* pMP = i < (int)vpMP.size() ? vpMP[i] : nullptr;
            if (pMP) ids[i] = (uint64_t)pMP->mnId;
        }
        // mvDepth travels with the keyframe like in the reference's serialisation (KeyFrame.h:68-79; UnprojectStereo reads it on the server); a keyframe
        // without the vector (monocular) files -1
        const float* pdepth = (int)pKF->mvDepth.size() == N ? pKF->mvDepth.data() : depth.data();
        check(corb_kf_store_put_host(store, slot, kp.data(), desc.data(), pKF->mvuRight.data(), pdepth, N, (uint64_t)pKF->mnId), "corb_kf_store_put_host");
        CorbKeyFrameMeta m; std::memset(&m, 0, sizeof(m));
        m.id = (uint64_t)pKF->mnId; m.client_id = clientId; m.flags = (pKF->isBad() ? CORB_KF_BAD : 0u) | (pKF->getFixed() ? CORB_KF_FIXED : 0u);
        m.fx = pKF->fx; m.fy = pKF->fy; m.cx = pKF->cx; m.cy = pKF->cy; m.bf = pKF->mbf;
        m.nlevels = (int32_t)std::min<size_t>(pKF->mvInvLevelSigma2.size(), 16);
        for (int l = 0; l < m.nlevels; l++) m.inv_level_sigma2[l] = pKF->mvInvLevelSigma2[l];
        const Mat T = pKF->GetPose();
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { m.Tcw[4 * r + c] = matf(T, r, c); m.TcwGBA[4 * r + c] = r == c ? 1.f : 0.f; }
        check(corb_kf_store_set_meta(store, slot, &m), "corb_kf_store_set_meta");
        check(corb_kf_store_set_map_points(store, slot, ids.data()), "corb_kf_store_set_map_points");
        const FeatureVector fv = flatten_featvec(pKF->mFeatVec);
        if (!fv.node_id.empty()) { CorbFeatVec c = fv.c(); check(corb_kf_store_set_bow(store, slot, &c), "corb_kf_store_set_bow"); }
    }
    // records first .. first + n of the map-point store: header fields of MapPoint.h:52-72 and mObservations as (keyframe mnId, feature index), ascending in
    // the keyframe id like the reference's std::map<LightKeyFrame, size_t>
    static void PutMapPoints(CorbMpStore* store, int first, const std::vector<MapPoint*>& vpMP, int clientId = 0)
    {
        std::vector<CorbMapPointRecord> rec(vpMP.size()); std::vector<int32_t> off(vpMP.size() + 1, 0); std::vector<uint64_t> okf; std::vector<uint32_t> oidx;
        for (size_t m = 0; m < vpMP.size(); m++) {
            MapPoint* pMP = vpMP[m]; CorbMapPointRecord& r = rec[m]; std::memset(&r, 0, sizeof(r));
            r.id = (uint64_t)pMP->mnId; r.client_id = clientId; r.flags = (pMP->isBad() ? CORB_MP_BAD : 0u) | (pMP->getFixed() ? CORB_MP_FIXED : 0u);
            if (auto* pRef = pMP->GetReferenceKeyFrame()) r.ref_kf_id = (uint64_t)pRef->mnId;      // mpRefKF (MapPoint.h:66)
            const Mat X = pMP->GetWorldPos();
            for (int a = 0; a < 3; a++) r.world_pos[a] = matf(X, a);
            std::vector<std::pair<uint64_t, uint32_t>> obs;
            const auto observations = pMP->GetObservations();
            for (auto it = observations.begin(); it != observations.end(); ++it) obs.emplace_back((uint64_t)it->first->mnId, (uint32_t)it->second);
            std::sort(obs.begin(), obs.end());
            for (auto& o : obs) { okf.push_back(o.first); oidx.push_back(o.second); }
            r.n_obs = (int32_t)obs.size(); off[m + 1] = (int32_t)okf.size();
        }
        check(corb_mp_store_put_host(store, first, (int)vpMP.size(), rec.data(), off.data(), okf.data(), oidx.data()), "corb_mp_store_put_host");
        // the public tracking / local-mapping / loop-closing fields the reference's archive moves as well (MapPoint.h:53-58, 151-174): they ride behind the lists
        std::vector<CorbMapPointScratch> sc(vpMP.size());
        for (size_t m = 0; m < vpMP.size(); m++) {
            MapPoint* pMP = vpMP[m]; CorbMapPointScratch& c = sc[m]; std::memset(&c, 0, sizeof(c));
            c.first_kf_id = (int64_t)pMP->mnFirstKFid; c.first_frame = (int64_t)pMP->mnFirstFrame; c.n_obs_weight = pMP->nObs;
            c.track_proj_x = pMP->mTrackProjX; c.track_proj_y = pMP->mTrackProjY; c.track_proj_xr = pMP->mTrackProjXR; c.track_view_cos = pMP->mTrackViewCos;
            c.track_in_view = pMP->mbTrackInView ? 1 : 0; c.track_scale_level = pMP->mnTrackScaleLevel;
            c.track_reference_for_frame = (uint64_t)pMP->mnTrackReferenceForFrame; c.last_frame_seen = (uint64_t)pMP->mnLastFrameSeen;
            c.ba_local_for_kf = (uint64_t)pMP->mnBALocalForKF; c.fuse_candidate_for_kf = (uint64_t)pMP->mnFuseCandidateForKF; c.loop_point_for_kf = (uint64_t)pMP->mnLoopPointForKF;
            c.corrected_by_kf = (uint64_t)pMP->mnCorrectedByKF; c.corrected_reference = (uint64_t)pMP->mnCorrectedReference;
        }
        if (!sc.empty()) check(corb_mp_store_set_scratch(store, first, (int)sc.size(), sc.data()), "corb_mp_store_set_scratch");
    }
    // the same fields back into the objects (the receiving side of a push: what boost's load leaves in a MapPoint)
    static void ReadBackScratch(CorbMpStore* store, int first, const std::vector<MapPoint*>& vpMP)
    {
        std::vector<CorbMapPointScratch> sc(vpMP.size());
        if (sc.empty()) return;
        check(corb_mp_store_get_scratch(store, first, (int)sc.size(), sc.data()), "corb_mp_store_get_scratch");
        for (size_t m = 0; m < vpMP.size(); m++) {
            MapPoint* pMP = vpMP[m]; const CorbMapPointScratch& c = sc[m];
            pMP->mnFirstKFid = (long int)c.first_kf_id; pMP->mnFirstFrame = (long int)c.first_frame; pMP->nObs = c.n_obs_weight;
            pMP->mTrackProjX = c.track_proj_x; pMP->mTrackProjY = c.track_proj_y; pMP->mTrackProjXR = c.track_proj_xr; pMP->mTrackViewCos = c.track_view_cos;
            pMP->mbTrackInView = c.track_in_view != 0; pMP->mnTrackScaleLevel = c.track_scale_level;
            pMP->mnTrackReferenceForFrame = (long unsigned int)c.track_reference_for_frame; pMP->mnLastFrameSeen = (long unsigned int)c.last_frame_seen;
            pMP->mnBALocalForKF = (long unsigned int)c.ba_local_for_kf; pMP->mnFuseCandidateForKF = (long unsigned int)c.fuse_candidate_for_kf; pMP->mnLoopPointForKF = (long unsigned int)c.loop_point_for_kf;
            pMP->mnCorrectedByKF = (long unsigned int)c.corrected_by_kf; pMP->mnCorrectedReference = (long unsigned int)c.corrected_reference;
        }
    }
    // Optimizer::GlobalBundleAdjustemnt(pCache, nIterations, pbStopFlag, nLoopKF, bRobust) on records (GlobalOptimize.cpp:444 on the server rank)
    // scaleFactor (ORBextractor's, KeyFrame::mfScaleFactor) > 0 and nLoopKF == 0: the write-back also does pMP->UpdateNormalAndDepth() on the records (Optimizer.cc:254-256)
    static CorbBAResult GlobalBundleAdjustemnt(CorbKfStore* kf, const std::vector<int32_t>& kfSlots, CorbMpStore* mp, const std::vector<int32_t>& mpSlots, int nIterations = 5,
                                               bool* pbStopFlag = nullptr, const unsigned long nLoopKF = 0, const bool bRobust = true, float scaleFactor = 0.f)
    {
        CorbBAResult r{};
        StopBridge stop(pbStopFlag);
        CorbBAOptions opt{}; opt.scale_factor = scaleFactor;
        check(corb_ba_solve_store(kf, kfSlots.data(), (int)kfSlots.size(), mp, mpSlots.data(), (int)mpSlots.size(), nIterations, bRobust ? 1 : 0, stop.ptr(pbStopFlag),
                                  (uint64_t)nLoopKF, &r, &opt), "corb_ba_solve_store");
        return r;
    }
    // void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Cache* pCache) (Optimizer.cc:487-838) on records: the caller selects the window as the
    // reference does (:493-546) and names it by slots -- lLocalKeyFrames, lFixedCameras, lLocalMapPoints; scaleFactor = pKF->mfScaleFactor.  The records receive the
    // poses / positions, vToErase (with SetBadFlag below three observations) and UpdateNormalAndDepth; vToErase (optional) lists the erased observations as
    // (index into localKfSlots ++ fixedKfSlots, index into mpSlots) for ReadBackLocalBA.
    static CorbBAResult LocalBundleAdjustment(CorbKfStore* kf, const std::vector<int32_t>& localKfSlots, const std::vector<int32_t>& fixedKfSlots, CorbMpStore* mp,
                                              const std::vector<int32_t>& mpSlots, float scaleFactor, bool* pbStopFlag = nullptr,
                                              std::vector<std::pair<int32_t, int32_t>>* vToErase = nullptr, bool applyErase = true)
    {
        CorbBAResult r{};
        StopBridge stop(pbStopFlag);
        std::vector<int32_t> slots(localKfSlots); slots.insert(slots.end(), fixedKfSlots.begin(), fixedKfSlots.end());
        const float hm = std::sqrt(5.991f), hs = std::sqrt(7.815f);
        const CorbBAStage st[2] = { {5, 1, 5.991f, 7.815f, 1, 0, 0, 0, 0, hm, hs}, {10, 0, 5.991f, 7.815f, 1, 0, 1, 0, 0, hm, hs} };      // optimize(5) / classify / optimize(10) / final test on every edge (:711-790)
        std::vector<int32_t> pairs(2 * std::max<size_t>(1, slots.size() * mpSlots.size())); int n = 0;
        check(corb_local_ba_store(kf, slots.data(), (int)localKfSlots.size(), (int)slots.size(), mp, mpSlots.data(), (int)mpSlots.size(), st, 2, scaleFactor, applyErase ? 1 : 0,
                                  stop.ptr(pbStopFlag), &r, pairs.data(), (int)(pairs.size() / 2), &n, nullptr), "corb_local_ba_store");
        if (vToErase) { vToErase->clear(); for (int k = 0; k < n; k++) vToErase->emplace_back(pairs[2 * k], pairs[2 * k + 1]); }
        return r;
    }
    // what LocalBundleAdjustment leaves in the records -> the objects (Optimizer.cc:796-836): the erased observations first, then the local keyframes' poses and the
    // local points' positions (+ UpdateNormalAndDepth on the object, as the reference calls it)
    static void ReadBackLocalBA(CorbKfStore* kf, const std::vector<int32_t>& localKfSlots, const std::vector<KeyFrame*>& vpLocalAndFixedKF, CorbMpStore* mp, int first,
                                const std::vector<MapPoint*>& vpMP, const std::vector<std::pair<int32_t, int32_t>>& vToErase)
    {
        for (const auto& e : vToErase) { KeyFrame* pKFi = vpLocalAndFixedKF[e.first]; MapPoint* pMPi = vpMP[e.second]; pKFi->EraseMapPointMatch(pMPi); pMPi->EraseObservation(pKFi); }
        for (size_t k = 0; k < localKfSlots.size(); k++) ReadBackKeyFrame(kf, localKfSlots[k], vpLocalAndFixedKF[k], 0);
        std::vector<CorbMapPointRecord> rec(vpMP.size());
        check(corb_mp_store_get(mp, first, (int)vpMP.size(), rec.data(), nullptr, nullptr), "corb_mp_store_get");
        for (size_t m = 0; m < vpMP.size(); m++) {
            MapPoint* pMP = vpMP[m];
            if (pMP->getFixed()) continue;                                            // if (!pMP->getFixed()) (:826)
            pMP->SetWorldPos(MatFactory<Mat>::from_floats(3, 1, rec[m].world_pos)); pMP->getCache()->addUpdateMapPoint(pMP); pMP->UpdateNormalAndDepth();
        }
    }
    // the record's estimate -> the object (Optimizer.cc:216-237): a record the solve did not write keeps what PutKeyFrame filed, so the copy is idempotent
    static void ReadBackKeyFrame(CorbKfStore* store, int slot, KeyFrame* pKF, const unsigned long nLoopKF)
    {
        CorbKeyFrameMeta m; check(corb_kf_store_get_meta(store, slot, &m), "corb_kf_store_get_meta");
        if (pKF->isBad() || pKF->getFixed()) return;
        if (nLoopKF == 0) { pKF->SetPose(MatFactory<Mat>::from_floats(4, 4, m.Tcw)); pKF->mpCacher->addUpdateKeyframe(pKF); }
        else if (m.ba_global_for_kf == (uint64_t)nLoopKF) { pKF->mTcwGBA = MatFactory<Mat>::from_floats(4, 4, m.TcwGBA); pKF->mnBAGlobalForKF = nLoopKF; }
    }
    // (:240-262) -- `optimised[m]`: the point had an edge in the solve (ba_global_for_kf == nLoopKF says so for nLoopKF != 0; for nLoopKF == 0 the caller
    // knows it from the observation lists it filed: a point without observations among the solve's keyframes is not touched)
    static void ReadBackMapPoints(CorbMpStore* store, int first, const std::vector<MapPoint*>& vpMP, const unsigned long nLoopKF, const std::vector<uint8_t>& optimised)
    {
        std::vector<CorbMapPointRecord> rec(vpMP.size());
        check(corb_mp_store_get(store, first, (int)vpMP.size(), rec.data(), nullptr, nullptr), "corb_mp_store_get");
        for (size_t m = 0; m < vpMP.size(); m++) {
            MapPoint* pMP = vpMP[m];
            if (pMP->isBad() || pMP->getFixed()) continue;
            if (nLoopKF == 0) { if (!optimised[m]) continue; pMP->SetWorldPos(MatFactory<Mat>::from_floats(3, 1, rec[m].world_pos)); pMP->getCache()->addUpdateMapPoint(pMP); pMP->UpdateNormalAndDepth(); }
            else if (rec[m].ba_global_for_kf == (uint64_t)nLoopKF) { pMP->mPosGBA = MatFactory<Mat>::from_floats(3, 1, rec[m].pos_gba); pMP->mnBAGlobalForKF = nLoopKF; }
        }
    }
};


// ---- the moment a tracked frame becomes a keyframe, on records (include/corb_keyframe_insert.h) ----
//   Tracking::CreateNewKeyFrame / StereoInitialization / UpdateLastFrame's point creation     Tracking.cc:1096-1158, 524-540, 830-883
//   LocalMapping::ProcessNewKeyFrame's association loop                                          LocalMapping.cc:132-151
//   LocalMapping::MapPointCulling                                                                LocalMapping.cc:161-188
// The keyframe / frame is the record MapStoreT::PutKeyFrame (or a front-end) filed in `slot`; nothing is flattened but ids and slots.  One object per client: it owns
// the calls' device scratch (CorbKfInsert).  A CORB_ERR_CAPACITY answer is thrown like every other error: nothing was written.
template <class KeyFrame, class MapPoint>
class KeyFrameInsertT {
public:
    KeyFrameInsertT(int maxFeatures, int maxRecent, int device = 0) { check(corb_kfi_create(device, maxFeatures, maxRecent, &h_), "corb_kfi_create"); }
    KeyFrameInsertT(const KeyFrameInsertT&) = delete; KeyFrameInsertT& operator=(const KeyFrameInsertT&) = delete;
    ~KeyFrameInsertT() { if (h_) corb_kfi_destroy(h_); }
    CorbKfInsert* handle() const { return h_; }

    // vOrder[j] = feature of visited entry j, vKind[j] (1, 2: created), vX3D = 3 floats per created point: the k-th is record firstMpSlot + k with id firstMpId + k
    struct StereoPoints { std::vector<int32_t> vOrder; std::vector<uint8_t> vKind; std::vector<float> vX3D; int nCreated = 0; };
    // F = pKF (KeyFrame*, modes 0 / 1) or the last Frame (mode 2): only its N is read, the features are the record's
    template <class FrameLike>
    StereoPoints CreateStereoPoints(const FrameLike& F, CorbKfStore* kf, int slot, CorbMpStore* map, const CorbTrackCamera& cam, float thDepth, int mode, bool apply,
                                    int firstMpSlot, uint64_t firstMpId, int clientId, long frameId, CorbKfStore* mirror = nullptr, int mirrorSlot = -1)
    {
        const size_t N = (size_t)std::max(F.N, 1);
        StereoPoints o; o.vOrder.resize(N); o.vKind.resize(N); o.vX3D.resize(3 * N);
        int nVisited = 0;
        check(corb_kfi_create_stereo_points(h_, kf, slot, map, &cam, thDepth, mode, apply ? 1 : 0, firstMpSlot, firstMpId, clientId, (int64_t)frameId, mirror, mirrorSlot,
                                            o.vOrder.data(), o.vKind.data(), o.vX3D.data(), &nVisited, &o.nCreated), "corb_kfi_create_stereo_points");
        o.vOrder.resize((size_t)nVisited); o.vKind.resize((size_t)nVisited); o.vX3D.resize(3 * (size_t)o.nCreated);
        return o;
    }
    // nTrackedClose, nNonTrackedClose (Tracking.cc:1026-1035) of the frame record; nRefMatches = mpReferenceKF->TrackedMapPoints(nMinObs) of record refSlot
    struct KeyFrameCounts { int nTrackedClose = 0, nNonTrackedClose = 0, nRefMatches = 0; };
    KeyFrameCounts NeedNewKeyFrameCounts(CorbKfStore* frames, int curSlot, CorbMpStore* map, float thDepth, CorbKfStore* kf, int refSlot, int nMinObs, int kfFirst, int kfN)
    {
        KeyFrameCounts c;
        check(corb_kfi_need_keyframe_counts(h_, frames, curSlot, map, thDepth, kf, refSlot, nMinObs, kfFirst, kfN, &c.nTrackedClose, &c.nNonTrackedClose, &c.nRefMatches),
              "corb_kfi_need_keyframe_counts");
        return c;
    }
    // vKind per feature (3: the observation was added), vRecentSlots = the map-point slots that enter mlpRecentAddedMapPoints, in feature order
    struct Association { std::vector<uint8_t> vKind; std::vector<int32_t> vRecentSlots; int nAdded = 0; };
    Association ProcessNewKeyFrame(KeyFrame* pKF, CorbKfStore* kf, int slot, CorbMpStore* map, int kfFirst, int kfN, float scaleFactor, bool apply)
    {
        const size_t N = (size_t)std::max(pKF->N, 1);
        Association o; o.vKind.resize(N); o.vRecentSlots.resize(N);
        int nRecent = 0;
        check(corb_kfi_process_new_keyframe(h_, kf, slot, map, kfFirst, kfN, scaleFactor, apply ? 1 : 0, o.vKind.data(), o.vRecentSlots.data(), &o.nAdded, &nRecent),
              "corb_kfi_process_new_keyframe");
        o.vKind.resize((size_t)pKF->N); o.vRecentSlots.resize((size_t)nRecent);
        return o;
    }
    // mlpRecentAddedMapPoints is walked as the reference walks it: an entry whose decision is not 0 leaves the list.  slotOf(pMP) = its record's slot.  Returns the
    // decisions in list order (2, 3: SetBadFlag was done on the records when apply; the objects are the caller's to mark).
    template <class SlotOf>
    std::vector<uint8_t> MapPointCulling(std::list<MapPoint*>& lRecent, SlotOf slotOf, CorbMpStore* map, unsigned long nCurrentKFid, bool bMonocular, CorbKfStore* kf,
                                         int kfFirst, int kfN, bool apply)
    {
        std::vector<int32_t> slots; slots.reserve(lRecent.size());
        for (MapPoint* pMP : lRecent) slots.push_back((int32_t)slotOf(pMP));
        std::vector<uint8_t> decision(std::max<size_t>(slots.size(), 1)); std::vector<int32_t> kept(std::max<size_t>(slots.size(), 1));
        int nKept = 0, nCulled = 0;
        check(corb_kfi_map_point_culling(h_, map, slots.data(), (int)slots.size(), (uint64_t)nCurrentKFid, bMonocular ? 2 : 3, kf, kfFirst, kfN, apply ? 1 : 0,
                                         decision.data(), kept.data(), &nKept, &nCulled), "corb_kfi_map_point_culling");
        decision.resize(slots.size());
        size_t i = 0;
        for (auto lit = lRecent.begin(); lit != lRecent.end(); i++) { if (decision[i] != 0) lit = lRecent.erase(lit); else ++lit; }
        return decision;
    }
private:
    CorbKfInsert* h_ = nullptr;
};

// ---- the server's detection loop on records (include/corb_map_fusion.h) ----
//   bool MapFusion::detectKeyFrameInServerMap(pMap, tKF, Tcw, candidateKFs)        S/src/MapFusion.cpp:660-756, called per keyframe by mapFuseToGlobalMap / mapFuse :432-620
// Detect() walks the keyframes of a submap as that loop walks them, with the argument meaning of the reference: for each keyframe the candidates of
// DetectMapFusionCandidatesFromDB, SearchByBoWInServer(0.75, true) against each, the candidates that are bad / have fewer than 15 matches discarded, PnPsolver with
// SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) on the rest and iterate(5) round-robin until a solver returns a pose (a refined one, or with bNoMore its best
// hypothesis on record: the reference takes any non-empty Tcw) -- and stops at the first keyframe that yields
// one.  On records that is ONE corb_map_fusion_candidates_store for the whole submap, then one corb_pnp_ransac_store per keyframe in order (it takes the kept rows' ids
// where the first call left them) with corb::pnp_replay answering the iterate(5) calls.  The keyframes are named by their records: subSlotOf(pKF) in `sub`,
// entrySlot[e] in `global` for database entry e.  Pose refinement, SearchByProjection and ComputeSim3 after a pose stay where they are (corb_track_*, corb_sim3_*).
template <class KeyFrame, class Db>
class MapFusionDetectT {
public:
    struct Params { float nnratio = 0.75f; bool checkOrientation = true; int minMatches = 15; double probability = 0.99; int minInliers = 10, maxIterations = 300, minSet = 4;
                    float epsilon = 0.5f, th2 = 5.991f; int nIterations = 5, tailIterations = 0; };
    struct Detection {
        FusionCandidates cand;                   // every keyframe's rows, whether the walk reached it or not
        int iKeyFrame = -1;                      // the first keyframe that yielded a pose (-1: none), its row among all rows, and the solver's answer
        int row = -1;
        bool bRefined = false;                   // the pose is Refine()'s (mRefinedTcw); false: the running best returned with bNoMore (mBestTcw, PnPsolver.cc:286-299)
        float Tcw[16] = {0};                     // the Tcw iterate() returned
        std::vector<uint8_t> vbInliers;          // per feature of that keyframe: mvbRefinedInliers or mvbBestInliers
        int nTried = 0;                          // keyframes that had a PnP call
    };
    // rand(k) -> the k-th draw of one keyframe's solvers (the reference draws from rand(); here the draws are data: RANSAC routes, DESIGN)
    template <class SubSlotOf, class Rand>
    Detection Detect(const std::vector<KeyFrame*>& vpKFs, SubSlotOf subSlotOf, Db& db, CorbKfStore* sub, CorbKfStore* global, const std::vector<int32_t>& entrySlot,
                     CorbMpStore* map, const CorbTrackCamera& cam, Rand rand, int capRows, int64_t capIds, const Params& P = Params())
    {
        std::vector<int32_t> slots, entries; std::vector<uint64_t> ids;
        for (KeyFrame* p : vpKFs) { slots.push_back((int32_t)subSlotOf(p)); entries.push_back(db.Entry(p)); ids.push_back((uint64_t)p->mnId); }
        Detection d;
        d.cand = MapFusionCandidates(db.handle(), sub, slots, entries, ids, global, entrySlot, capRows, capIds, P.nnratio, P.checkOrientation, P.minMatches);
        const int stride = P.maxIterations + P.tailIterations;
        for (size_t i = 0; i < vpKFs.size() && d.iKeyFrame < 0; i++) {
            const int r0 = d.cand.rowOffset[i], r1 = d.cand.rowOffset[i + 1];
            std::vector<int> kept; for (int r = r0; r < r1; r++) if (d.cand.rows[r].kept) kept.push_back(r);
            if (kept.empty()) continue;                                                   // every candidate discarded (:700-707)
            const int n = corb_kf_store_count(sub, slots[i]), nc = (int)kept.size();
            if (n <= 0) continue;
            std::vector<int32_t> rv((size_t)nc * stride * P.minSet); for (size_t k = 0; k < rv.size(); k++) rv[k] = (int32_t)rand(k);
            std::vector<int32_t> cap(nc), mi(nc), nrec(nc), ncorr(nc), counts((size_t)nc * stride);
            std::vector<CorbPnPRansacRecord> rec((size_t)nc * stride); std::vector<uint8_t> bf((size_t)nc * stride * n), rf((size_t)nc * stride * n);
            check(corb_pnp_ransac_store(sub, slots[i], map, &cam, d.cand.ids.data() + d.cand.rows[kept[0]].ids_offset, nc, P.probability, P.minInliers, P.maxIterations, P.minSet,
                                        P.epsilon, P.th2, P.tailIterations, rv.data(), stride, cap.data(), mi.data(), nrec.data(), rec.data(), bf.data(), rf.data(), ncorr.data(),
                                        nullptr, counts.data(), nullptr, nullptr), "corb_pnp_ransac_store");
            d.nTried++;
            // the round-robin of :709-752: iterate(nIterations) per live solver until one returns a pose or all are discarded
            std::vector<int> its(nc, 0); std::vector<char> dead(nc, 0); int alive = nc;
            while (alive > 0 && d.iKeyFrame < 0)
                for (int c = 0; c < nc && d.iKeyFrame < 0; c++) {
                    if (dead[c]) continue;
                    const int k = std::min(nrec[c], stride);
                    const PnPReplay a = pnp_replay(counts.data() + (size_t)c * stride, stride, rec.data() + (size_t)c * stride, k, mi[c], cap[c], its[c], P.nIterations);
                    its[c] = a.iterations;
                    if (a.kind != PnPReplay::Refined) { dead[c] = 1; alive--; }           // bNoMore: vbDiscarded[i] = true (:728-732)
                    if (a.kind == PnPReplay::None) continue;                              // an empty Tcw
                    // any pose ends the walk (:735-741): Refine()'s, or -- with bNoMore -- the best hypothesis on record whose Refine() never succeeded
                    d.bRefined = a.kind == PnPReplay::Refined;
                    d.iKeyFrame = (int)i; d.row = kept[c];
                    const size_t at = (size_t)c * stride + a.record;
                    const float* T = d.bRefined ? rec[at].Tcw_refined : rec[at].Tcw_best;
                    for (int j = 0; j < 12; j++) d.Tcw[j] = T[j];
                    d.Tcw[12] = d.Tcw[13] = d.Tcw[14] = 0.f; d.Tcw[15] = 1.f;
                    const std::vector<uint8_t>& fl = d.bRefined ? rf : bf;
                    d.vbInliers.assign(fl.begin() + at * n, fl.begin() + (at + 1) * n);
                }
        }
        return d;
    }
};

// ---- the server -> clients publish on records (include/corb_map_publish.h) ----
//   server: MapFusion::runPubTopic / resentGlobalMapToClient -> PubToClient::pub*ToClients             S/src/MapFusion.cpp:315-430, S/src/PubToClient.cpp:24-163
//   client: Cache::subNewInsertKeyFramesFromServer / subNewInsertMapPointFromServer / subUpdated*      C/src/Cache.cc:446-634
// One object per rank: it owns the message buffer and the calls' device scratch (CorbMapPublisher).  resentGlobalMapToClient is Pack fed 50 keyframe and 2000
// map-point handles per round.
template <class Mat>
class MapPublishT {
public:
    explicit MapPublishT(int device = 0) { check(corb_pub_create(device, &h_), "corb_pub_create"); }
    MapPublishT(const MapPublishT&) = delete; MapPublishT& operator=(const MapPublishT&) = delete;
    ~MapPublishT() { if (h_) corb_pub_destroy(h_); }
    CorbMapPublisher* handle() const { return h_; }

    // the four sets and transMs -> slot lists and the table.  A set is any ordered container of light handles with mnId (std::set<LightKeyFrame> iterates in
    // ascending id, and so do the slot lists); kfSlotOf(id) / mpSlotOf(id) = the slot of the server's record, negative for a handle the cache does not resolve,
    // which is skipped as `if( tKF )` skips it (PubToClient.cpp:32-33).
    struct PackLists { std::vector<int32_t> newKF, updKF, newMP, updMP, clientIds; std::vector<float> trans; };
    template <class KFSet, class MPSet, class KfSlotOf, class MpSlotOf>
    static PackLists Lists(const KFSet& newKFs, const MPSet& newMPs, const KFSet& updKFs, const MPSet& updMPs, KfSlotOf kfSlotOf, MpSlotOf mpSlotOf, const std::map<int, Mat>& transMs)
    {
        PackLists L;
        for (const auto& l : newKFs) { const int s = (int)kfSlotOf(l.mnId); if (s >= 0) L.newKF.push_back(s); }
        for (const auto& l : newMPs) { const int s = (int)mpSlotOf(l.mnId); if (s >= 0) L.newMP.push_back(s); }
        for (const auto& l : updKFs) { const int s = (int)kfSlotOf(l.mnId); if (s >= 0) L.updKF.push_back(s); }
        for (const auto& l : updMPs) { const int s = (int)mpSlotOf(l.mnId); if (s >= 0) L.updMP.push_back(s); }
        for (const auto& t : transMs) { L.clientIds.push_back((int32_t)t.first); for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) L.trans.push_back(matf(t.second, r, c)); }
        return L;
    }
    template <class KFSet, class MPSet, class KfSlotOf, class MpSlotOf>
    void Pack(CorbKfStore* kf, CorbMpStore* mp, const KFSet& newKFs, const MPSet& newMPs, const KFSet& updKFs, const MPSet& updMPs, KfSlotOf kfSlotOf, MpSlotOf mpSlotOf,
              const std::map<int, Mat>& transMs)
    {
        const PackLists L = Lists(newKFs, newMPs, updKFs, updMPs, kfSlotOf, mpSlotOf, transMs);
        check(corb_pub_pack(h_, kf, L.newKF.data(), (int)L.newKF.size(), L.updKF.data(), (int)L.updKF.size(), mp, L.newMP.data(), (int)L.newMP.size(), L.updMP.data(),
                            (int)L.updMP.size(), L.clientIds.data(), L.trans.data(), (int)L.clientIds.size()), "corb_pub_pack");
    }
    struct Message { void* ptr = nullptr; int64_t bytes = 0; int32_t counts[5] = {0, 0, 0, 0, 0}; int32_t kfRecordBytes = 0, mpRecordBytes = 0; };
    Message GetMessage() const
    {
        Message m; check(corb_pub_message(h_, &m.ptr, &m.bytes, m.counts, &m.kfRecordBytes, &m.mpRecordBytes), "corb_pub_message");
        return m;
    }
    // what the four callbacks did with a message: kinds per entry (A, B: 1 own, 2 held, 3 accepted; C, D: 0 unknown, 1 not fixed, 2 moved), the slots the accepted
    // records went to, in message order.  The caller then does addKeyFrametoDB / AddKeyFrameFromServer for vNewKFSlots on its own structures: corb_kfdb_add for the
    // keyframe database entry, corb_covis_update for the covisibility rows (Cache.cc:483-484).  bFull: CORB_ERR_CAPACITY -- nothing was written.
    struct Applied { std::vector<uint8_t> vKindNewKF, vKindNewMP, vKindUpdKF, vKindUpdMP; std::vector<int32_t> vNewKFSlots, vNewMPSlots; int nUpdatedKF = 0, nUpdatedMP = 0; bool bNoTransform = false, bFull = false; };
    Applied Apply(const Message& m, int clientId, CorbKfStore* kf, int kfFirst, int kfN, int kfFreeFirst, int kfRoom, CorbMpStore* mp, int mpFirst, int mpN, int mpFreeFirst, int mpRoom,
                  bool apply = true)
    {
        Applied a;
        a.vKindNewKF.resize((size_t)std::max(m.counts[0], 1)); a.vKindNewMP.resize((size_t)std::max(m.counts[1], 1)); a.vKindUpdKF.resize((size_t)std::max(m.counts[2], 1));
        a.vKindUpdMP.resize((size_t)std::max(m.counts[3], 1)); a.vNewKFSlots.resize((size_t)std::max(std::min(m.counts[0], kfRoom), 1)); a.vNewMPSlots.resize((size_t)std::max(std::min(m.counts[1], mpRoom), 1));
        CorbPublishOutputs o; std::memset(&o, 0, sizeof(o));
        o.kind_kf_new = a.vKindNewKF.data(); o.kind_mp_new = a.vKindNewMP.data(); o.kind_kf_upd = a.vKindUpdKF.data(); o.kind_mp_upd = a.vKindUpdMP.data();
        o.kf_new_slots = a.vNewKFSlots.data(); o.mp_new_slots = a.vNewMPSlots.data();
        const int rc = corb_pub_apply(h_, m.ptr, m.counts, m.kfRecordBytes, m.mpRecordBytes, clientId, kf, kfFirst, kfN, kfFreeFirst, kfRoom, mp, mpFirst, mpN, mpFreeFirst, mpRoom,
                                      apply ? 1 : 0, &o);
        if (rc != CORB_ERR_CAPACITY) check(rc, "corb_pub_apply");
        a.bFull = rc == CORB_ERR_CAPACITY; a.bNoTransform = o.no_transform != 0; a.nUpdatedKF = o.n_kf_updated; a.nUpdatedMP = o.n_mp_updated;
        a.vKindNewKF.resize((size_t)m.counts[0]); a.vKindNewMP.resize((size_t)m.counts[1]); a.vKindUpdKF.resize((size_t)m.counts[2]); a.vKindUpdMP.resize((size_t)m.counts[3]);
        a.vNewKFSlots.resize((size_t)std::min(o.n_kf_inserted, std::min(m.counts[0], kfRoom))); a.vNewMPSlots.resize((size_t)std::min(o.n_mp_inserted, std::min(m.counts[1], mpRoom)));
        return a;
    }
private:
    CorbMapPublisher* h_ = nullptr;
};

// ---- the tracking thread on device-resident records (corb_track_*, include/corb_accel.h): a Frame lives in a slot of a keyframe store, the client's map in a
// map-point store; the calls below are Tracking::TrackWithMotionModel / TrackLocalMap's matcher and optimiser calls with the reference's argument meaning.
// MapPoint needs two accessors the reference does not have (the raw mfMinDistance / mfMaxDistance next to Get*DistanceInvariance()): GetMinDistance(), GetMaxDistance().
// what Tracking::UpdateLocalMap leaves (corb_track_update_local_map): mvpLocalKeyFrames / mvpLocalMapPoints as slots of the graph's stores, the points' ids as
// SearchLocalPoints sends them, and pKFmax (refSlot -1: mpReferenceKF stays)
struct LocalMapSlots { std::vector<int32_t> kfSlots, mpSlots; std::vector<uint64_t> mpIds; int nVoted = 0, refSlot = -1, nCleared = 0; bool counterEmpty = false; };
inline LocalMapSlots UpdateLocalMapSlots(CorbCovis* graph, CorbKfStore* frames, int slot, const std::vector<int32_t>& prevKfSlots, int maxKeyFrames, int maxMapPoints)
{
    LocalMapSlots r; CorbLocalMap info; std::memset(&info, 0, sizeof(info));
    r.kfSlots.resize((size_t)std::max(maxKeyFrames, 1)); r.mpSlots.resize((size_t)std::max(maxMapPoints, 1)); r.mpIds.resize((size_t)std::max(maxMapPoints, 1));
    check(corb_track_update_local_map(graph, frames, slot, prevKfSlots.data(), (int)prevKfSlots.size(), r.kfSlots.data(), maxKeyFrames, r.mpSlots.data(), r.mpIds.data(), maxMapPoints, &info),
          "corb_track_update_local_map");
    r.kfSlots.resize((size_t)info.n_kf); r.mpSlots.resize((size_t)info.n_mp); r.mpIds.resize((size_t)info.n_mp);
    r.nVoted = info.n_voted; r.refSlot = info.ref_slot; r.nCleared = info.n_cleared; r.counterEmpty = info.counter_empty != 0;
    return r;
}

template <class Frame, class MapPoint, class Mat> struct FrameStoreT {
    // void Tracking::UpdateLocalMap() for the Frame in `slot` of `store` (Tracking.cc:1218-1366): the lists as slots and ids; the frame's record loses its bad points
    // (ReadBackMapPoints brings that into the Frame).  corb::Covisibility::UpdateLocalMap answers KeyFrame pointers.
    static LocalMapSlots UpdateLocalMap(CorbCovis* graph, CorbKfStore* store, int slot, const std::vector<int32_t>& prevKfSlots, int maxKeyFrames, int maxMapPoints)
    {
        return UpdateLocalMapSlots(graph, store, slot, prevKfSlots, maxKeyFrames, maxMapPoints);
    }
    // void Tracking::SearchLocalPoints() with mvpLocalMapPoints as the ids UpdateLocalMap returned
    static int SearchLocalPoints(CorbKfStore* store, int slot, CorbMpStore* map, const Frame& F, const std::vector<uint64_t>& localPointIds, const float th, float nnratio = 0.8f, int* nToMatch = nullptr)
    {
        float Tcw[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw[4 * r + c] = matf(F.mTcw, r, c);
        const CorbTrackCamera cam = Camera(F);
        int n = 0, nv = 0;
        check(corb_track_search_local_points(store, slot, map, localPointIds.data(), (int)localPointIds.size(), &cam, Tcw, F.mfLogScaleFactor, th, nnratio, nullptr, nullptr, &n, &nv), "corb_track_search_local_points");
        if (nToMatch) *nToMatch = nv;
        return n;
    }
    static CorbTrackCamera Camera(const Frame& F)
    {
        CorbTrackCamera c; std::memset(&c, 0, sizeof(c));
        c.fx = F.fx; c.fy = F.fy; c.cx = F.cx; c.cy = F.cy; c.bf = F.mbf; c.mb = F.mb;
        c.min_x = Frame::mnMinX; c.max_x = Frame::mnMaxX; c.min_y = Frame::mnMinY; c.max_y = Frame::mnMaxY;
        c.nlevels = (int32_t)std::min<size_t>(F.mvScaleFactors.size(), 16);
        for (int l = 0; l < c.nlevels; l++) c.scale[l] = F.mvScaleFactors[l];
        return c;
    }
    // the Frame's features, pose, mvInvLevelSigma2, mvpMapPoints (as ids) and mvbOutlier -> record `slot`
    static void PutFrame(CorbKfStore* store, int slot, const Frame& F)
    {
        const int N = F.N;
        std::vector<CorbKeyPoint> kp(N); std::vector<uint8_t> desc((size_t)N * 32), fl(N, 0); std::vector<uint64_t> ids(N, CORB_NO_MAP_POINT);
        for (int i = 0; i < N; i++) {
            const auto& k = F.mvKeysUn[i];
            kp[i] = CorbKeyPoint{k.pt.x, k.pt.y, k.size, k.angle, k.response, k.octave, k.class_id};
            std::memcpy(&desc[(size_t)i * 32], F.mDescriptors.template ptr<uint8_t>(i), 32);
            MapPoint* pMP = F.mvpMapPoints[i].getMapPoint();
            if (pMP) ids[i] = (uint64_t)pMP->mnId;
            if (i < (int)F.mvbOutlier.size() && F.mvbOutlier[i]) fl[i] = 2;                    // record feature flag bit 1 = mvbOutlier
        }
        CorbKeyFrameMeta m; std::memset(&m, 0, sizeof(m));
        m.id = (uint64_t)F.mnId; m.fx = F.fx; m.fy = F.fy; m.cx = F.cx; m.cy = F.cy; m.bf = F.mbf;
        m.nlevels = (int32_t)std::min<size_t>(F.mvInvLevelSigma2.size(), 16);
        for (int l = 0; l < m.nlevels; l++) m.inv_level_sigma2[l] = F.mvInvLevelSigma2[l];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { m.Tcw[4 * r + c] = F.mTcw.empty() ? (r == c ? 1.f : 0.f) : matf(F.mTcw, r, c); m.TcwGBA[4 * r + c] = r == c ? 1.f : 0.f; }
        check(corb_kf_store_put_frame(store, slot, kp.data(), desc.data(), F.mvuRight.data(), nullptr, N, &m), "corb_kf_store_put_frame");
        check(corb_kf_store_set_map_points(store, slot, ids.data()), "corb_kf_store_set_map_points");
        check(corb_kf_store_set_flags(store, slot, fl.data()), "corb_kf_store_set_flags");
    }
    // the client's map: MapStoreT::PutMapPoints' fields plus what the tracking calls read (normal, distance range, descriptor), then the id index
    static void PutMap(CorbMpStore* store, const std::vector<MapPoint*>& vpMP)
    {
        std::vector<CorbMapPointRecord> rec(vpMP.size()); std::vector<int32_t> off(vpMP.size() + 1, 0); std::vector<uint64_t> okf; std::vector<uint32_t> oidx;
        for (size_t m = 0; m < vpMP.size(); m++) {
            MapPoint* pMP = vpMP[m]; CorbMapPointRecord& r = rec[m]; std::memset(&r, 0, sizeof(r));
            r.id = (uint64_t)pMP->mnId; r.flags = pMP->isBad() ? CORB_MP_BAD : 0u;
            const Mat X = pMP->GetWorldPos(), Nn = pMP->GetNormal(), D = pMP->GetDescriptor();
            for (int a = 0; a < 3; a++) { r.world_pos[a] = matf(X, a); r.normal[a] = Nn.empty() ? 0.f : matf(Nn, a); }
            r.min_distance = pMP->GetMinDistance(); r.max_distance = pMP->GetMaxDistance();
            if (!D.empty()) std::memcpy(r.descriptor, D.template ptr<uint8_t>(0), 32);
            const auto observations = pMP->GetObservations();
            std::vector<std::pair<uint64_t, uint32_t>> obs;
            for (auto it = observations.begin(); it != observations.end(); ++it) obs.emplace_back((uint64_t)it->first->mnId, (uint32_t)it->second);
            std::sort(obs.begin(), obs.end());
            for (auto& o : obs) { okf.push_back(o.first); oidx.push_back(o.second); }
            r.n_obs = (int32_t)obs.size(); off[m + 1] = (int32_t)okf.size();
        }
        check(corb_mp_store_put_host(store, 0, (int)vpMP.size(), rec.data(), off.data(), okf.data(), oidx.data()), "corb_mp_store_put_host");
        check(corb_mp_store_build_index(store, 0, (int)vpMP.size()), "corb_mp_store_build_index");
    }
    // int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono): CurrentFrame.mTcw = the predicted pose
    static int SearchByProjection(CorbKfStore* store, int curSlot, int lastSlot, CorbMpStore* map, const Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono,
                                  float nnratio = 0.9f, bool checkOri = true)
    {
        float Tcw[16], Tlw[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { Tcw[4 * r + c] = matf(CurrentFrame.mTcw, r, c); Tlw[4 * r + c] = matf(LastFrame.mTcw, r, c); }
        const CorbTrackCamera cam = Camera(CurrentFrame);
        int n = 0;
        check(corb_track_search_last_frame(store, curSlot, lastSlot, map, Tcw, Tlw, &cam, th, bMono ? 1 : 0, nnratio, checkOri ? 1 : 0, nullptr, &n), "corb_track_search_last_frame");
        return n;
    }
    // int Optimizer::PoseOptimization(Frame *pFrame) (+ the caller's "Discard outliers" loop when discardOutliers): pose and mvbOutlier land in the Frame as well
    static int PoseOptimization(CorbKfStore* store, int slot, CorbMpStore* map, Frame* pFrame, bool discardOutliers)
    {
        float Tin[16], Tout[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tin[4 * r + c] = matf(pFrame->mTcw, r, c);
        const CorbTrackCamera cam = Camera(*pFrame);
        std::vector<uint8_t> o((size_t)std::max(pFrame->N, 1)); int32_t inl = 0;
        check(corb_track_pose_optimization(store, slot, map, &cam, Tin, Tout, discardOutliers ? 1 : 0, o.data(), &inl), "corb_track_pose_optimization");
        pFrame->SetPose(MatFactory<Mat>::from_floats(4, 4, Tout));
        pFrame->mvbOutlier.assign(pFrame->N, false);
        typedef typename std::decay<decltype(pFrame->mvpMapPoints[0])>::type LMP;
        for (int i = 0; i < pFrame->N; i++) if (o[i]) { if (discardOutliers) pFrame->mvpMapPoints[i] = LMP{nullptr}; else pFrame->mvbOutlier[i] = true; }
        return inl;
    }
    // void Tracking::SearchLocalPoints(): returns the matches; *nToMatch = the points that passed isInFrustum
    static int SearchLocalPoints(CorbKfStore* store, int slot, CorbMpStore* map, const Frame& F, const std::vector<MapPoint*>& vpLocalMapPoints, const float th, float nnratio = 0.8f, int* nToMatch = nullptr)
    {
        std::vector<uint64_t> ids(vpLocalMapPoints.size());
        for (size_t i = 0; i < ids.size(); i++) ids[i] = (uint64_t)vpLocalMapPoints[i]->mnId;
        float Tcw[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw[4 * r + c] = matf(F.mTcw, r, c);
        const CorbTrackCamera cam = Camera(F);
        int n = 0, nv = 0;
        check(corb_track_search_local_points(store, slot, map, ids.data(), (int)ids.size(), &cam, Tcw, F.mfLogScaleFactor, th, nnratio, nullptr, nullptr, &n, &nv), "corb_track_search_local_points");
        if (nToMatch) *nToMatch = nv;
        return n;
    }
    // bool Tracking::TrackLocalMap() (Tracking.cc:951-992) for the Frame in `slot` of `store` in ONE call (corb_track_local_map): UpdateLocalMap, SearchLocalPoints,
    // PoseOptimization and the tail; mnVisible / mnFound and the tracking fields of the MapPoints are written on their records.  The Tracking members the function
    // reads travel in `tracking` (mSensor as System::eSensor's value, mbOnlyTracking, mnLastRelocFrameId, mMaxFrames).  The Frame receives the pose and mvbOutlier;
    // ReadBackMapPoints brings mvpMapPoints over.  *pOut (optional): the lists, the matches and the counts (mnMatchesInliers = result.n_matches_inliers).
    struct TrackingState { int mSensor = 1; bool mbOnlyTracking = false; uint64_t mnLastRelocFrameId = 0; int mMaxFrames = 30; };
    static bool TrackLocalMap(CorbCovis* graph, CorbKfStore* store, int slot, Frame* pFrame, const TrackingState& tracking, const std::vector<int32_t>& prevKfSlots,
                              int maxKeyFrames, int maxMapPoints, TrackLocalMapOutput* pOut = nullptr, float nnratio = 0.8f)
    {
        float Tin[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tin[4 * r + c] = matf(pFrame->mTcw, r, c);
        const CorbTrackCamera cam = Camera(*pFrame);
        CorbTrackLocalMapParams p; std::memset(&p, 0, sizeof(p));
        p.frame_id = (uint64_t)pFrame->mnId; p.last_reloc_frame_id = tracking.mnLastRelocFrameId; p.max_frames = tracking.mMaxFrames; p.sensor = tracking.mSensor;
        p.only_tracking = tracking.mbOnlyTracking ? 1 : 0; p.log_scale_factor = pFrame->mfLogScaleFactor; p.nnratio = nnratio; p.th = 0.f;
        TrackLocalMapOutput o = corb::TrackLocalMap(graph, store, slot, cam, Tin, prevKfSlots, p, maxKeyFrames, maxMapPoints);
        pFrame->SetPose(MatFactory<Mat>::from_floats(4, 4, o.result.Tcw));
        pFrame->mvbOutlier.assign(pFrame->N, false);
        for (int i = 0; i < pFrame->N; i++) if (o.outlier[i]) pFrame->mvbOutlier[i] = true;
        const bool ok = o.result.ok != 0;
        if (pOut) *pOut = std::move(o);
        return ok;
    }
    // the record's mvpMapPoints -> the Frame (ids resolved through the caller's id -> MapPoint* map; features whose point was discarded hold none)
    template <class Lookup> static void ReadBackMapPoints(CorbKfStore* store, int slot, Frame* pFrame, const Lookup& byId)
    {
        const int N = pFrame->N;
        std::vector<uint64_t> ids((size_t)std::max(N, 1)); std::vector<uint8_t> fl((size_t)std::max(N, 1));
        check(corb_kf_store_get_map_points(store, slot, ids.data(), N), "corb_kf_store_get_map_points");
        int n = 0; uint64_t kid = 0; int32_t nn = 0;
        check(corb_kf_store_get(store, slot, nullptr, nullptr, nullptr, nullptr, fl.data(), N, &n, &kid, nullptr, nullptr, nullptr, &nn), "corb_kf_store_get");
        typedef typename std::decay<decltype(pFrame->mvpMapPoints[0])>::type LMP;
        for (int i = 0; i < N; i++) {
            pFrame->mvpMapPoints[i] = LMP{nullptr};
            if (ids[i] != CORB_NO_MAP_POINT && !(fl[i] & 4)) { auto it = byId.find((unsigned long)ids[i]); if (it != byId.end()) pFrame->mvpMapPoints[i] = LMP{it->second}; }
        }
    }
};
}  // namespace adapt
}  // namespace corb

// ---- on a tree with the reference's headers: the reference's own class names ----
// ---- Sim3Solver (corbslam_client/include/Sim3Solver.h) over corb_sim3_ransac ----
// The reference's constructor and method signatures.  The constructor flattens as C/src/Sim3Solver.cc:43-109 do (GetMapPointMatches, isBad, GetIndexInKeyFrame,
// mvKeysUn[index].octave -> mvLevelSigma2, Rcw * Xw + tcw as cv::gemm computes it: double accumulation, one rounding; mK); the first iterate() pre-draws
// maxIterations x 3 values from the random source (a callable returning rand()'s range [0, 2^31); DUtils::Random::RandomInt consumes exactly one rand() per draw),
// makes ONE library call that evaluates every hypothesis, and iterate() is then replayed from the events: the position advances by nIterations, an event inside
// the window is returned, bNoMore is set when mRansacMaxIts is reached without a return.  Mat = the type KeyFrame::GetRotation() returns.
namespace corb {
template <class KeyFrame, class MapPoint>
class Sim3Solver {
public:
    using Mat = decltype(std::declval<KeyFrame&>().GetRotation());
    using RandomSource = std::function<int()>;
    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true, RandomSource rnd = [] { return std::rand(); }, int device = 0)
        : mbFixScale(bFixScale), rnd_(std::move(rnd)), device_(device)
    {
        check_abi();
        std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        const Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
        auto to_camera = [](const Mat& R, const Mat& t, const Mat& X, std::vector<float>& out) {
            for (int r = 0; r < 3; r++) {
                double s = (double)adapt::matf(R, r, 0) * (double)adapt::matf(X, 0);
                s = s + (double)adapt::matf(R, r, 1) * (double)adapt::matf(X, 1);
                s = s + (double)adapt::matf(R, r, 2) * (double)adapt::matf(X, 2);
                out.push_back((float)(s + (double)adapt::matf(t, r)));
            }
        };
        for (int i1 = 0; i1 < mN1; i1++) {
            if (!vpMatched12[i1]) continue;
            MapPoint* pMP1 = vpKeyFrameMP1[i1]; MapPoint* pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            sigma2_1_.push_back(pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave]);
            sigma2_2_.push_back(pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave]);
            mvnIndices1.push_back((size_t)i1);
            to_camera(Rcw1, tcw1, pMP1->GetWorldPos(), p1c_); to_camera(Rcw2, tcw2, pMP2->GetWorldPos(), p2c_);
        }
        N = (int)mvnIndices1.size();
        const Mat K1 = pKF1->mK, K2 = pKF2->mK;
        problem_.fx1 = adapt::matf(K1, 0, 0); problem_.fy1 = adapt::matf(K1, 1, 1); problem_.cx1 = adapt::matf(K1, 0, 2); problem_.cy1 = adapt::matf(K1, 1, 2);
        problem_.fx2 = adapt::matf(K2, 0, 0); problem_.fy2 = adapt::matf(K2, 1, 1); problem_.cx2 = adapt::matf(K2, 0, 2); problem_.cy2 = adapt::matf(K2, 1, 2);
        SetRansacParameters();
    }
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mRansacProb = probability; mRansacMinInliers = minInliers; maxIterations_ = maxIterations;
        mnIterations = 0; ready_ = false; last_ = -1;
    }
    Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        bNoMore = false; vbInliers = std::vector<bool>(mN1, false); nInliers = 0;
        if (N < mRansacMinInliers) { bNoMore = true; return Mat(); }
        run();
        const int end = std::min(mnIterations + std::max(nIterations, 0), mRansacMaxIts);
        for (int k = 0; k < (int)events_.size(); k++) {
            const CorbSim3RansacEvent& e = events_[k];
            if (e.iteration <= mnIterations || e.iteration > end) continue;
            mnIterations = e.iteration; last_ = k; nInliers = e.n_inliers;
            for (int i = 0; i < N; i++) if (flags_[(size_t)k * N + i]) vbInliers[mvnIndices1[i]] = true;
            float T[16] = {e.s12 * e.R12[0], e.s12 * e.R12[1], e.s12 * e.R12[2], e.t12[0], e.s12 * e.R12[3], e.s12 * e.R12[4], e.s12 * e.R12[5], e.t12[1],
                           e.s12 * e.R12[6], e.s12 * e.R12[7], e.s12 * e.R12[8], e.t12[2], 0.f, 0.f, 0.f, 1.f};
            return adapt::MatFactory<Mat>::from_floats(4, 4, T);
        }
        mnIterations = end;
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return Mat();
    }
    Mat find(std::vector<bool>& vbInliers12, int& nInliers)
    {
        bool bFlag;
        if (N >= mRansacMinInliers) run();
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }
    // the best model so far; every caller reads them after iterate() returned a transformation, and they are that return's
    Mat GetEstimatedRotation() { return last_ < 0 ? Mat() : adapt::MatFactory<Mat>::from_floats(3, 3, events_[last_].R12); }
    Mat GetEstimatedTranslation() { return last_ < 0 ? Mat() : adapt::MatFactory<Mat>::from_floats(3, 1, events_[last_].t12); }
    float GetEstimatedScale() { return last_ < 0 ? 1.0f : events_[last_].s12; }

private:
    void run()
    {
        if (ready_) return;
        std::vector<int32_t> rv((size_t)std::max(maxIterations_, 0) * 3);
        for (auto& v : rv) v = (int32_t)rnd_();
        problem_.n = N; problem_.p1c = p1c_.data(); problem_.p2c = p2c_.data(); problem_.sigma2_1 = sigma2_1_.data(); problem_.sigma2_2 = sigma2_2_.data();
        const int me = std::max(maxIterations_, 1); int32_t cap = 0, n_ev = 0;
        events_.assign((size_t)me, CorbSim3RansacEvent()); flags_.assign((size_t)me * std::max(N, 1), 0);
        check(corb_sim3_ransac(&problem_, 1, mRansacProb, mRansacMinInliers, maxIterations_, mbFixScale ? 1 : 0, rv.data(), me, std::max(N, 1), &cap, &n_ev, events_.data(),
                               flags_.data(), nullptr, nullptr, device_), "corb_sim3_ransac");
        mRansacMaxIts = cap; events_.resize((size_t)std::min<int>(n_ev, me)); ready_ = true;
    }
    int N = 0, mN1 = 0, mnIterations = 0, mRansacMinInliers = 6, mRansacMaxIts = 0, maxIterations_ = 300, last_ = -1;
    double mRansacProb = 0.99; bool mbFixScale, ready_ = false;
    std::vector<size_t> mvnIndices1; std::vector<float> p1c_, p2c_, sigma2_1_, sigma2_2_;
    CorbSim3RansacProblem problem_{}; std::vector<CorbSim3RansacEvent> events_; std::vector<uint8_t> flags_;
    RandomSource rnd_; int device_;
};
}  // namespace corb

// ---- PnPsolver (corbslam_client/include/PnPsolver.h) over corb_pnp_ransac ----
// The reference's constructors (over a Frame, C/src/PnPsolver.cc:67-110, and over a KeyFrame, :112-155) and method signatures.  The constructor flattens as the
// reference's does (vpMapPointMatches[i] non-NULL and not bad; mvKeysUn[i].pt, mvLevelSigma2[octave], GetWorldPos(), fx / fy / cx / cy).  The first iterate() pre-draws
// (maxIterations + tail_iterations) x minSet values from the random source (a callable returning rand()'s range [0, 2^31)), makes ONE library call that evaluates
// every hypothesis and every Refine(), and iterate() is then replayed by corb::pnp_replay.  The reference's loop runs on behind mRansacMaxIts for as long as it is
// called (:227); here mRansacMaxIts + tail_iterations hypotheses exist and iterate() reports bNoMore once they run out.  PnPsolver::RunBatch evaluates all candidates
// of a relocalisation in one call.  Mat = the type MapPoint::GetWorldPos() returns.
namespace corb {
template <class Frame, class KeyFrame, class MapPoint>
class PnPsolver {
public:
    using Mat = decltype(std::declval<MapPoint&>().GetWorldPos());
    using RandomSource = std::function<int()>;
    PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches, RandomSource rnd = [] { return std::rand(); }, int tail_iterations = 0, int device = 0)
        : rnd_(std::move(rnd)), tail_(tail_iterations), device_(device) { init(F, vpMapPointMatches); }
    PnPsolver(const KeyFrame& F, const std::vector<MapPoint*>& vpMapPointMatches, RandomSource rnd = [] { return std::rand(); }, int tail_iterations = 0, int device = 0)
        : rnd_(std::move(rnd)), tail_(tail_iterations), device_(device) { init(F, vpMapPointMatches); }
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991)
    {
        mRansacProb = probability; minInliers_ = minInliers; maxIterations_ = maxIterations; mRansacMinSet = minSet; epsilon_ = epsilon; th2_ = th2;
        mnIterations = 0; ready_ = false;
    }
    Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        RunBatch({this});
        bNoMore = false; vbInliers.clear(); nInliers = 0;
        if (mRansacMaxIts == 0) { bNoMore = true; return Mat(); }                 // N < mRansacMinInliers (:218-222)
        const PnPReplay r = pnp_replay(counts_.data(), mRansacMaxIts + tail_, records_.data(), (int)records_.size(), mRansacMinInliers, mRansacMaxIts, mnIterations, nIterations);
        mnIterations = r.iterations;
        if (r.kind == PnPReplay::None) { bNoMore = true; return Mat(); }
        const bool refined = r.kind == PnPReplay::Refined;
        const CorbPnPRansacRecord& e = records_[r.record];
        bNoMore = !refined; nInliers = refined ? e.n_refined : e.n_inliers;
        vbInliers = std::vector<bool>(n_matches_, false);
        const uint8_t* fl = (refined ? refined_flags_ : best_flags_).data() + (size_t)r.record * std::max(N, 1);
        for (int i = 0; i < N; i++) if (fl[i]) vbInliers[mvKeyPointIndices[i]] = true;
        const float* T = refined ? e.Tcw_refined : e.Tcw_best;
        const float T16[16] = {T[0], T[1], T[2], T[3], T[4], T[5], T[6], T[7], T[8], T[9], T[10], T[11], 0.f, 0.f, 0.f, 1.f};
        return adapt::MatFactory<Mat>::from_floats(4, 4, T16);
    }
    Mat find(std::vector<bool>& vbInliers, int& nInliers)
    {
        bool bFlag;
        RunBatch({this});
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }
    // every solver of `solvers` that has not run yet, in ONE corb_pnp_ransac call per set of equal parameters (Tracking::Relocalization: all candidate keyframes)
    static void RunBatch(const std::vector<PnPsolver*>& solvers)
    {
        std::vector<PnPsolver*> todo;
        for (PnPsolver* s : solvers) if (s && !s->ready_) todo.push_back(s);
        while (!todo.empty()) {
            PnPsolver* h = todo.front(); std::vector<PnPsolver*> grp, rest;
            for (PnPsolver* s : todo)
                (s->mRansacProb == h->mRansacProb && s->minInliers_ == h->minInliers_ && s->maxIterations_ == h->maxIterations_ && s->mRansacMinSet == h->mRansacMinSet &&
                 s->epsilon_ == h->epsilon_ && s->th2_ == h->th2_ && s->tail_ == h->tail_ && s->device_ == h->device_ ? grp : rest).push_back(s);
            const int n = (int)grp.size(), stride_its = std::max(h->maxIterations_, 0) + std::max(h->tail_, 0), me = std::max(stride_its, 1);
            std::vector<CorbPnPRansacProblem> pr((size_t)n); std::vector<int32_t> rv((size_t)n * stride_its * std::max(h->mRansacMinSet, 0));
            int stride = 1;
            for (int c = 0; c < n; c++) {
                PnPsolver* s = grp[c];
                for (size_t k = 0; k < (size_t)stride_its * std::max(h->mRansacMinSet, 0); k++) rv[(size_t)c * stride_its * h->mRansacMinSet + k] = (int32_t)s->rnd_();
                pr[c].n = s->N; pr[c].p3dw = s->p3dw_.data(); pr[c].p2d = s->p2d_.data(); pr[c].sigma2 = s->sigma2_.data();
                pr[c].fx = s->fx_; pr[c].fy = s->fy_; pr[c].cx = s->cx_; pr[c].cy = s->cy_;
                stride = std::max(stride, s->N);
            }
            std::vector<int32_t> cap((size_t)n), mi((size_t)n), n_rec((size_t)n), counts((size_t)n * me);
            std::vector<CorbPnPRansacRecord> rec((size_t)n * me); std::vector<uint8_t> bf((size_t)n * me * stride), rf((size_t)n * me * stride);
            check(corb_pnp_ransac(pr.data(), n, h->mRansacProb, h->minInliers_, h->maxIterations_, h->mRansacMinSet, h->epsilon_, h->th2_, h->tail_, rv.data(), me, stride,
                                  cap.data(), mi.data(), n_rec.data(), rec.data(), bf.data(), rf.data(), counts.data(), nullptr, nullptr, h->device_), "corb_pnp_ransac");
            for (int c = 0; c < n; c++) {
                PnPsolver* s = grp[c]; const int k = std::min<int>(n_rec[c], me), w = std::max(s->N, 1);
                s->mRansacMaxIts = cap[c]; s->mRansacMinInliers = mi[c];
                s->counts_.assign(counts.begin() + (size_t)c * me, counts.begin() + (size_t)(c + 1) * me);
                s->records_.assign(rec.begin() + (size_t)c * me, rec.begin() + (size_t)c * me + k);
                s->best_flags_.assign((size_t)k * w, 0); s->refined_flags_.assign((size_t)k * w, 0);
                for (int r = 0; r < k; r++)
                    for (int i = 0; i < s->N; i++) {
                        s->best_flags_[(size_t)r * w + i] = bf[((size_t)c * me + r) * stride + i]; s->refined_flags_[(size_t)r * w + i] = rf[((size_t)c * me + r) * stride + i];
                    }
                s->ready_ = true;
            }
            todo.swap(rest);
        }
    }

private:
    template <class F> void init(const F& frame, const std::vector<MapPoint*>& vpMapPointMatches)
    {
        check_abi();
        n_matches_ = vpMapPointMatches.size();
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            MapPoint* pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            const auto& kp = frame.mvKeysUn[i];
            p2d_.push_back(kp.pt.x); p2d_.push_back(kp.pt.y);
            sigma2_.push_back(frame.mvLevelSigma2[kp.octave]);
            const Mat Pos = pMP->GetWorldPos();
            for (int k = 0; k < 3; k++) p3dw_.push_back(adapt::matf(Pos, k));
            mvKeyPointIndices.push_back(i);
        }
        N = (int)mvKeyPointIndices.size();
        fx_ = frame.fx; fy_ = frame.fy; cx_ = frame.cx; cy_ = frame.cy;
        SetRansacParameters();
    }
    int N = 0, mnIterations = 0, mRansacMinInliers = 0, mRansacMaxIts = 0, mRansacMinSet = 4, minInliers_ = 8, maxIterations_ = 300;
    double mRansacProb = 0.99; float epsilon_ = 0.4f, th2_ = 5.991f, fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0; bool ready_ = false; size_t n_matches_ = 0;
    std::vector<size_t> mvKeyPointIndices; std::vector<float> p3dw_, p2d_, sigma2_;
    std::vector<int32_t> counts_; std::vector<CorbPnPRansacRecord> records_; std::vector<uint8_t> best_flags_, refined_flags_;
    RandomSource rnd_; int tail_, device_;
};
}  // namespace corb

// ---- Initializer (corbslam_client/include/Initializer.h) over corb_mono_initialize ----
// The reference's constructor (C/src/Initializer.cc:33-42: mK and mvKeysUn of the reference frame, sigma, iterations) and Initialize signature (:44-45).  Each
// Initialize draws iterations x 8 values from the random source (a callable returning rand()'s range [0, 2^31)) in the order the source consumes rand() at :82-97 and
// makes ONE library call; Initializer::RunBatch evaluates the (reference, current) pairs of several clients in one call and Result() then hands each its answer.
// Mat = the type of Frame::mK; the points go into any vector of a type with float x, y, z.
namespace corb {
template <class Frame>
class Initializer {
public:
    using Mat = typename std::decay<decltype(std::declval<const Frame&>().mK)>::type;
    using RandomSource = std::function<int()>;
    struct Job { Initializer* init; const Frame* current; const std::vector<int>* vMatches12; };
    Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200, RandomSource rnd = [] { return std::rand(); }, int device = 0)
        : mSigma(sigma), mMaxIterations(iterations), rnd_(std::move(rnd)), device_(device)
    {
        check_abi();
        fx_ = adapt::matf(ReferenceFrame.mK, 0, 0); fy_ = adapt::matf(ReferenceFrame.mK, 1, 1); cx_ = adapt::matf(ReferenceFrame.mK, 0, 2); cy_ = adapt::matf(ReferenceFrame.mK, 1, 2);
        for (const auto& k : ReferenceFrame.mvKeysUn) { CorbKeyPoint o{}; o.x = k.pt.x; o.y = k.pt.y; mvKeys1.push_back(o); }
    }
    template <class Point3f>
    bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, Mat& R21, Mat& t21, std::vector<Point3f>& vP3D, std::vector<bool>& vbTriangulated)
    {
        RunBatch({Job{this, &CurrentFrame, &vMatches12}});
        return Result(R21, t21, vP3D, vbTriangulated);
    }
    // what the last Initialize / RunBatch left for this initializer; R21, t21, vP3D and vbTriangulated are written on success only, as in the source
    template <class Point3f>
    bool Result(Mat& R21, Mat& t21, std::vector<Point3f>& vP3D, std::vector<bool>& vbTriangulated) const
    {
        if (result.status != CORB_INIT_OK) return false;
        R21 = adapt::MatFactory<Mat>::from_floats(3, 3, result.R21); t21 = adapt::MatFactory<Mat>::from_floats(3, 1, result.t21);
        vP3D.resize(mvKeys1.size()); vbTriangulated.assign(mvKeys1.size(), false);
        for (size_t i = 0; i < mvKeys1.size(); i++) { vP3D[i].x = p3d_[3 * i]; vP3D[i].y = p3d_[3 * i + 1]; vP3D[i].z = p3d_[3 * i + 2]; vbTriangulated[i] = tri_[i] != 0; }
        return true;
    }
    // every job in ONE corb_mono_initialize call per set of equal parameters (the server runs one client per robot)
    static void RunBatch(const std::vector<Job>& jobs)
    {
        std::vector<Job> todo(jobs);
        while (!todo.empty()) {
            const Initializer* h = todo.front().init; std::vector<Job> grp, rest;
            for (const Job& j : todo) (j.init->mSigma == h->mSigma && j.init->mMaxIterations == h->mMaxIterations && j.init->device_ == h->device_ ? grp : rest).push_back(j);
            const int n = (int)grp.size(), its = std::max(h->mMaxIterations, 0);
            std::vector<CorbInitProblem> pr((size_t)n); std::vector<std::vector<CorbKeyPoint>> keys2((size_t)n); std::vector<std::vector<int32_t>> m12((size_t)n);
            std::vector<int32_t> rv((size_t)n * its * 8);
            int stride = 1;
            for (int c = 0; c < n; c++) {
                Initializer* s = grp[c].init;
                for (const auto& k : grp[c].current->mvKeysUn) { CorbKeyPoint o{}; o.x = k.pt.x; o.y = k.pt.y; keys2[c].push_back(o); }
                m12[c].assign(s->mvKeys1.size(), -1);                  // vMatches12 is indexed by the reference frame's keys (:54-63)
                for (size_t i = 0; i < grp[c].vMatches12->size() && i < m12[c].size(); i++) m12[c][i] = (*grp[c].vMatches12)[i];
                for (int k = 0; k < its * 8; k++) rv[(size_t)c * its * 8 + k] = (int32_t)s->rnd_();
                pr[c].keys1 = s->mvKeys1.data(); pr[c].n1 = (int32_t)s->mvKeys1.size(); pr[c].keys2 = keys2[c].data(); pr[c].n2 = (int32_t)keys2[c].size();
                pr[c].matches12 = m12[c].data(); pr[c].fx = s->fx_; pr[c].fy = s->fy_; pr[c].cx = s->cx_; pr[c].cy = s->cy_;
                stride = std::max(stride, (int)s->mvKeys1.size());
            }
            std::vector<CorbInitResult> res((size_t)n); std::vector<float> p3d((size_t)n * stride * 3); std::vector<uint8_t> tri((size_t)n * stride);
            check(corb_mono_initialize(pr.data(), n, h->mSigma, h->mMaxIterations, 1.0f, 50, rv.data(), stride, 0, res.data(), p3d.data(), tri.data(), nullptr, nullptr, nullptr,
                                       h->device_), "corb_mono_initialize");                    // minParallax 1.0, minTriangulated 50 (:116-118)
            for (int c = 0; c < n; c++) {
                Initializer* s = grp[c].init; const size_t n1 = s->mvKeys1.size();
                s->result = res[c];
                s->p3d_.assign(p3d.begin() + (size_t)c * stride * 3, p3d.begin() + (size_t)c * stride * 3 + n1 * 3);
                s->tri_.assign(tri.begin() + (size_t)c * stride, tri.begin() + (size_t)c * stride + n1);
            }
            todo.swap(rest);
        }
    }
    CorbInitResult result{};                                           // every diagnostic of the last call

private:
    std::vector<CorbKeyPoint> mvKeys1; float mSigma; int mMaxIterations; float fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0;
    std::vector<float> p3d_; std::vector<uint8_t> tri_;
    RandomSource rnd_; int device_;
};
}  // namespace corb

// ---- place recognition: ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) and KeyFrameDatabase (include/KeyFrameDatabase.h:46-68) ----
//   void ORBVocabulary::transform(const vector<cv::Mat>&, DBoW2::BowVector&, DBoW2::FeatureVector&, int levelsup)   TemplatedVocabulary.h:1127
//   double ORBVocabulary::score(const BowVector&, const BowVector&)                                               :1199
//   void add(KeyFrame*) / erase(KeyFrame*) / clear()                                                               KeyFrameDatabase.cc:38-70
//   vector<KeyFrame*> DetectLoopCandidates(KeyFrame*, float minScore) / DetectRelocalizationCandidates(Frame*) / DetectMapFusionCandidatesFromDB(KeyFrame*)   :73-401
// The database maps KeyFrame* to entries of a CorbKfDb as it meets them: a keyframe's mBowVec is uploaded once (ComputeBoW computes it once), the six per-keyframe fields
// live in the device table (State() reads them), and GetBestCovisibilityKeyFrames(10) is read at add() and whenever the caller reports UpdateConnections().  The Frame of a
// relocalisation uses the table's last entry.  Two limits: an entry is given to a KeyFrame* once and kept after erase() (the reference's erased keyframes keep their
// fields, and neighbours may still name them), so capacity_keyframes bounds the keyframes ever met, not the live ones; and mBowVec is read at first sight only, so a
// keyframe must have its BoW computed before the database meets it (as KeyFrame's constructor guarantees in the reference).
namespace corb {
class ORBVocabulary {
public:
    ORBVocabulary() {}
    explicit ORBVocabulary(const std::string& text_file, int device = 0) { if (!loadFromTextFile(text_file, device)) throw Error(CORB_ERR_ARG, "ORBVocabulary"); }
    ORBVocabulary(const ORBVocabulary&) = delete; ORBVocabulary& operator=(const ORBVocabulary&) = delete;
    ~ORBVocabulary() { if (h_) corb_voc_destroy(h_); }
    bool loadFromTextFile(const std::string& path, int device = 0) { if (h_) { corb_voc_destroy(h_); h_ = nullptr; } return corb_voc_load_text(path.c_str(), device, &h_) == CORB_OK; }
    void create(const CorbVocDesc& d, int device = 0) { if (h_) { corb_voc_destroy(h_); h_ = nullptr; } check(corb_voc_create(&d, device, &h_), "corb_voc_create"); }
    // TemplatedVocabulary::create(training_features, k, L) (:592-600) on the device (include/corb_voc_train.h): one vector of descriptors per training image; `seed`
    // stands where the source seeds rand() from the clock, max_iterations bounds the k-means loop the source leaves unbounded (stats->capped_nodes tells)
    template <class Desc> void create(const std::vector<std::vector<Desc>>& training_features, int k, int L, uint64_t seed = 0, int max_iterations = 100, int device = 0, CorbVocTrainStats* stats = nullptr)
    {
        std::vector<int32_t> off(1, 0); std::vector<uint8_t> d;
        for (const auto& image : training_features) {
            for (const auto& f : image) { const uint8_t* r = adapt::desc_row(f, 0); d.insert(d.end(), r, r + 32); }
            off.push_back((int32_t)(d.size() / 32));
        }
        d.resize(d.size() + 32);
        const CorbVocTrainOptions o{k, L, max_iterations, 0, seed};
        if (h_) { corb_voc_destroy(h_); h_ = nullptr; }
        check(corb_voc_train(d.data(), off.data(), (int)training_features.size(), &o, device, &h_, stats), "corb_voc_train");
    }
    // saveToTextFile (:1429-1449): weight_digits 0 writes the source's bytes, 17 a file that reloads bit for bit
    void saveToTextFile(const std::string& path, int weight_digits = 0) const { check(corb_voc_save_text(h_, path.c_str(), weight_digits), "corb_voc_save_text"); }
    unsigned size() const { int32_t w = 0; if (h_) corb_voc_info(h_, nullptr, nullptr, nullptr, &w); return (unsigned)w; }
    bool empty() const { return size() == 0; }
    template <class Desc, class BowVec, class FeatVec> void transform(const std::vector<Desc>& features, BowVec& v, FeatVec& fv, int levelsup) const
    {
        v.clear(); fv.clear();
        const int n = (int)features.size();
        std::vector<uint8_t> d((size_t)n * 32 + 32);
        for (int i = 0; i < n; i++) std::memcpy(&d[(size_t)i * 32], adapt::desc_row(features[i], 0), 32);
        const int32_t off[2] = {0, n}; int32_t nw = 0, nn = 0;
        std::vector<uint32_t> w(n + 1), node(n + 1), idx(n + 1); std::vector<double> val(n + 1); std::vector<int32_t> fo(n + 2);
        check(corb_voc_transform(h_, d.data(), off, 1, levelsup, w.data(), val.data(), &nw, node.data(), fo.data(), idx.data(), &nn, nullptr, nullptr), "corb_voc_transform");
        for (int i = 0; i < nw; i++) v.insert(v.end(), std::make_pair(w[i], val[i]));
        for (int j = 0; j < nn; j++) { auto& g = fv[node[j]]; g.assign(idx.begin() + fo[j], idx.begin() + fo[j + 1]); }
    }
    // L1Scoring::score (ScoringObject.cpp:23-68) on two host vectors, as the source states it
    template <class BowVec> double score(const BowVec& v1, const BowVec& v2) const
    {
        auto i = v1.begin(), j = v2.begin(); double s = 0;
        while (i != v1.end() && j != v2.end()) {
            if (i->first == j->first) { s += std::fabs(i->second - j->second) - std::fabs(i->second) - std::fabs(j->second); ++i; ++j; }
            else if (i->first < j->first) i = v1.lower_bound(j->first);
            else j = v2.lower_bound(i->first);
        }
        return -s / 2.0;
    }
    CorbVoc* handle() const { return h_; }
private:
    CorbVoc* h_ = nullptr;
};

template <class KeyFrame, class Frame = KeyFrame>
class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary& voc, int capacity_keyframes, int max_words) : cap_(capacity_keyframes + 1), kf_((size_t)capacity_keyframes + 1, nullptr)
    { check(corb_kfdb_create(voc.handle(), cap_, max_words, &h_), "corb_kfdb_create"); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete; KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;
    ~KeyFrameDatabase() { if (h_) corb_kfdb_destroy(h_); }

    void add(KeyFrame* pKF) { const int e = entry(pKF); check(corb_kfdb_add(h_, e), "corb_kfdb_add"); UpdateConnections(pKF); }
    void erase(KeyFrame* pKF) { auto it = entry_.find(pKF); if (it != entry_.end()) check(corb_kfdb_erase(h_, it->second), "corb_kfdb_erase"); }
    void clear() { check(corb_kfdb_clear(h_), "corb_kfdb_clear"); }
    // to be called where the reference's covisibility graph changes (KeyFrame::UpdateConnections / UpdateBestCovisibles): re-reads GetBestCovisibilityKeyFrames(10)
    void UpdateConnections(KeyFrame* pKF)
    {
        const int32_t e = entry(pKF); int32_t row[10]; int m = 0;
        for (KeyFrame* p : pKF->GetBestCovisibilityKeyFrames(10)) if (m < 10) row[m++] = entry(p);
        for (; m < 10; m++) row[m] = -1;
        check(corb_kfdb_set_neighbours(h_, &e, 1, row), "corb_kfdb_set_neighbours");
    }
    std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore)
    {
        std::vector<int32_t> conn;
        for (KeyFrame* p : pKF->GetConnectedKeyFrames()) { auto it = entry_.find(p); if (it != entry_.end()) conn.push_back(it->second); }
        return detect(0, entry(pKF), (uint64_t)pKF->mnId, conn, minScore);
    }
    std::vector<KeyFrame*> DetectMapFusionCandidatesFromDB(KeyFrame* pKF) { return detect(2, entry(pKF), (uint64_t)pKF->mnId, {}, 0.f); }
    // DetectMapFusionCandidatesFromDB for every keyframe of a submap in one call (corb_kfdb_detect_batch): the lists the calls above give one after the other
    std::vector<std::vector<KeyFrame*>> DetectMapFusionCandidatesFromDB(const std::vector<KeyFrame*>& vpKFs)
    {
        std::vector<int32_t> e; std::vector<uint64_t> ids;
        for (KeyFrame* p : vpKFs) { e.push_back(entry(p)); ids.push_back((uint64_t)p->mnId); }
        const CandidateLists c = DetectBatch(h_, 2, e, ids, (int)std::min<size_t>(vpKFs.size() * (size_t)cap_, 1u << 30));
        std::vector<std::vector<KeyFrame*>> out(vpKFs.size());
        for (size_t i = 0; i < vpKFs.size(); i++) for (int k = c.offset[i]; k < c.offset[i + 1]; k++) out[i].push_back(kf_[c.cand[k]]);
        return out;
    }
    int Entry(KeyFrame* pKF) { return entry(pKF); }             // the keyframe's entry (its BowVector is uploaded at first sight)
    int Capacity() const { return cap_; }
    std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F)
    {
        set_bow(cap_ - 1, F->mBowVec);
        return detect(1, cap_ - 1, (uint64_t)F->mnId, {}, 0.f);
    }
    // the minScore loop of LoopClosing::DetectLoop (C/src/LoopClosing.cc:122-137): mpVoc->score(pKF->mBowVec, other->mBowVec) for each of `others`
    std::vector<double> Scores(KeyFrame* pKF, const std::vector<KeyFrame*>& others)
    {
        std::vector<int32_t> b; for (KeyFrame* p : others) b.push_back(entry(p));
        std::vector<double> s(b.size());
        check(corb_kfdb_score(h_, entry(pKF), b.data(), (int)b.size(), s.data()), "corb_kfdb_score");
        return s;
    }
    CorbKfDbState State(KeyFrame* pKF) const
    {
        CorbKfDbState s; std::memset(&s, 0, sizeof(s));
        auto it = entry_.find(pKF); if (it != entry_.end()) check(corb_kfdb_get_state(h_, it->second, 1, &s), "corb_kfdb_get_state");
        return s;
    }
    CorbKfDb* handle() const { return h_; }
private:
    template <class BowVec> void set_bow(int e, const BowVec& v)
    {
        std::vector<uint32_t> w; std::vector<double> val;
        for (auto it = v.begin(); it != v.end(); ++it) { w.push_back((uint32_t)it->first); val.push_back(it->second); }
        check(corb_kfdb_set_bow(h_, e, w.data(), val.data(), (int)w.size()), "corb_kfdb_set_bow");
    }
    int entry(KeyFrame* pKF)
    {
        auto it = entry_.find(pKF); if (it != entry_.end()) return it->second;
        if (next_ >= cap_ - 1) throw Error(CORB_ERR_CAPACITY, "KeyFrameDatabase: more keyframes than capacity_keyframes");
        const int e = next_++;
        set_bow(e, pKF->mBowVec); entry_[pKF] = e; kf_[e] = pKF;
        return e;
    }
    std::vector<KeyFrame*> detect(int kind, int q, uint64_t id, const std::vector<int32_t>& conn, float minScore)
    {
        std::vector<int32_t> out((size_t)cap_); int n = 0;
        check(corb_kfdb_detect(h_, kind, q, id, conn.data(), (int)conn.size(), minScore, out.data(), cap_, &n), "corb_kfdb_detect");
        std::vector<KeyFrame*> r; for (int i = 0; i < n; i++) r.push_back(kf_[out[i]]);
        return r;
    }
    CorbKfDb* h_ = nullptr; int cap_, next_ = 0;
    std::map<KeyFrame*, int> entry_; std::vector<KeyFrame*> kf_;
};

// ---- LoopClosing's queue and DetectLoop (C/src/LoopClosing.cc:87-231) on records: include/corb_loop_detect.h through corb::LoopDetector ----
//   void InsertKeyFrame(KeyFrame*)  :87-92 (mnId 0 is dropped)     bool CheckNewKeyFrames()  :94-98     bool DetectLoop()  :100-231
// The keyframes are named by their records: slotOf(pKF) in the graph's keyframe store; the database is the adapter above, whose entry of a keyframe is bound to its
// slot when the keyframe is first met here (InsertKeyFrame, or Bind for a keyframe that never passes the queue, such as mnId 0: every keyframe that can be covisible
// with a queued one needs its entry).  DetectLoop() hands the queue's front, up to maxQueue keyframes, to ONE corb_loop_detect_queue call and pops what that call
// consumed: it stops at the first detection, so a true return leaves mpCurrentKF and mvpEnoughConsistentCandidates as the reference's DetectLoop() leaves them for
// ComputeSim3, and the keyframes behind it still queued.  A false return means the chunk held no detection (more may be queued: CheckNewKeyFrames()).
// mvpEnoughConsistentCandidates is cleared where the reference clears it (:157): by a keyframe that had candidates.  GetBestCovisibilityKeyFrames(10) of the queued
// keyframes is read before the call, as KeyFrameDatabase::add reads it.  SetNotErase / SetErase stay with the caller.
namespace adapt {
template <class KeyFrame, class Db>
class LoopDetectT {
public:
    KeyFrame* mpCurrentKF = nullptr;
    std::vector<KeyFrame*> mvpEnoughConsistentCandidates;
    std::vector<KeyFrame*> vpCandidateKFs;               // of mpCurrentKF
    std::vector<LoopDetection> consumed;                 // what the last DetectLoop() call processed, in queue order
    template <class SlotOf>
    LoopDetectT(CorbCovis* graph, Db& db, SlotOf slotOf, int nSlots, int maxCandidates, int maxGroups, int maxQueue = 8)
        : det_(graph, db.handle(), maxCandidates, maxGroups), db_(db), slotOf_(slotOf), kfOfSlot_((size_t)nSlots, nullptr), maxQueue_(std::min(std::max(maxQueue, 1), CORB_LOOP_DETECT_MAX_QUEUE)) {}
    LoopDetector& detector() { return det_; }
    void Bind(KeyFrame* pKF)
    {
        const int s = slotOf_(pKF);
        if (s < 0 || s >= (int)kfOfSlot_.size()) throw Error(CORB_ERR_ARG, "LoopDetectT::Bind: the keyframe has no slot");
        if (kfOfSlot_[(size_t)s] == pKF) return;
        if (kfOfSlot_[(size_t)s]) det_.DropSlot(s);      // another keyframe takes the slot: the one before can never match again
        det_.Bind({s}, {db_.Entry(pKF)}); kfOfSlot_[(size_t)s] = pKF;
    }
    void InsertKeyFrame(KeyFrame* pKF) { Bind(pKF); if (pKF->mnId != 0) queue_.push_back(pKF); }        // :90
    bool CheckNewKeyFrames() const { return !queue_.empty(); }
    size_t QueueSize() const { return queue_.size(); }
    void SetLastLoop(KeyFrame* pKF) { det_.SetLastLoop((uint64_t)pKF->mnId); }                          // mLastLoopKFid = mpCurrentKF->mnId (:591)
    void ResetIfRequested() { queue_.clear(); det_.Reset(); }                                           // :644-648
    bool DetectLoop()
    {
        consumed.clear();
        if (queue_.empty()) return false;
        const size_t n = std::min(queue_.size(), (size_t)maxQueue_);
        std::vector<int32_t> slots;
        for (size_t k = 0; k < n; k++) { db_.UpdateConnections(queue_[k]); slots.push_back(slotOf_(queue_[k])); }
        consumed = det_.DetectLoopQueue(slots);
        bool detected = false;
        for (size_t k = 0; k < consumed.size(); k++) {
            const LoopDetection& d = consumed[k];
            mpCurrentKF = queue_[k];
            vpCandidateKFs.clear();
            for (int32_t s : d.candSlots) vpCandidateKFs.push_back(s >= 0 && s < (int)kfOfSlot_.size() ? kfOfSlot_[(size_t)s] : nullptr);
            if (d.result.n_candidates > 0) {
                mvpEnoughConsistentCandidates.clear();
                for (int32_t i : d.enough) mvpEnoughConsistentCandidates.push_back(vpCandidateKFs[(size_t)i]);
            }
            detected = d.detected();
        }
        queue_.erase(queue_.begin(), queue_.begin() + (std::ptrdiff_t)consumed.size());
        return detected;
    }
private:
    LoopDetector det_; Db& db_; std::function<int(KeyFrame*)> slotOf_; std::vector<KeyFrame*> kfOfSlot_; std::deque<KeyFrame*> queue_; int maxQueue_;
};
}  // namespace adapt
}  // namespace corb

// ---- covisibility graph: what KeyFrame::UpdateConnections and its readers do, on the records (corb_covis_*) ----
//   void KeyFrame::UpdateConnections()                                            KeyFrame.cc:404-502
//   vector<KeyFrame*> GetVectorCovisibleKeyFrames() / GetBestCovisibilityKeyFrames(N) / GetCovisiblesByWeight(w); int GetWeight(KeyFrame*)   :199-269
//   void LocalMapping::KeyFrameCulling()                                          LocalMapping.cc:590-648 (the decisions; SetBadFlag stays with the caller)
//   the window of Optimizer::LocalBundleAdjustment                                Optimizer.cc:493-544 (as the slot lists MapStoreT::LocalBundleAdjustment takes)
//   AddChild / EraseChild / ChangeParent / GetChilds / GetParent / hasChild and the tree part of SetBadFlag      KeyFrame.cc:504-543, :607-668
//   void Tracking::UpdateLocalMap()                                               Tracking.cc:1218-1366
//   CorrectLoop's propagation and the map update of RunGlobalBundleAdjustment      GlobalOptimize.cpp:253-338, :463-532 (LoopClosing.cc:436-522, :684-753)
//   AddLoopEdge / GetLoopEdges and Optimizer::OptimizeEssentialGraph                KeyFrame.cc:545-561, Optimizer.cc:840-1117 (include/corb_essential_graph.h)
// The keyframes are named by the slots MapStoreT::PutKeyFrame filed them in (Bind).  The spanning tree lives in the graph (corb_covis_update keeps it as :493-499 do);
// UpdateConnections still returns the front of the ordered list, which is mpParent on a keyframe's first connection.  Db (optional) is the place-recognition database of this header: its
// UpdateConnections(KeyFrame*) is called for the keyframe and for every keyframe on its ordered list -- the rows an update can change the best ten of.
namespace corb {
template <class KeyFrame, class Db>
class Covisibility {
public:
    struct Culling { KeyFrame* pKF; int nMPs, nRedundantObservations; bool bCull; };
    Covisibility(CorbKfStore* kf, CorbMpStore* mp, int max_connections = 0, Db* db = nullptr) : db_(db) { check(corb_covis_create(kf, mp, max_connections, &h_), "corb_covis_create"); }
    Covisibility(const Covisibility&) = delete; Covisibility& operator=(const Covisibility&) = delete;
    ~Covisibility() { if (h_) corb_covis_destroy(h_); }
    void Bind(KeyFrame* pKF, int slot) { slot_[pKF] = slot; if ((int)kf_.size() <= slot) kf_.resize((size_t)slot + 1, nullptr); kf_[slot] = pKF; }
    int Slot(KeyFrame* pKF) const { auto it = slot_.find(pKF); if (it == slot_.end()) throw Error(CORB_ERR_ARG, "Covisibility: keyframe without a slot (Bind)"); return it->second; }

    KeyFrame* UpdateConnections(KeyFrame* pKF, int th = 15)
    {
        const int32_t s = Slot(pKF); uint64_t first = CORB_NO_MAP_POINT;
        check(corb_covis_update(h_, &s, 1, th, &first), "corb_covis_update");
        const std::vector<KeyFrame*> listed = GetVectorCovisibleKeyFrames(pKF);
        if (db_) { db_->UpdateConnections(pKF); for (KeyFrame* p : listed) db_->UpdateConnections(p); }
        return first == CORB_NO_MAP_POINT || listed.empty() ? nullptr : listed.front();
    }
    // the connection part of KeyFrame::SetBadFlag (KeyFrame.cc:592-595, :604-605)
    void EraseConnections(KeyFrame* pKF) { check(corb_covis_erase(h_, Slot(pKF)), "corb_covis_erase"); }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames(KeyFrame* pKF) { return query(pKF, 0, 0); }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(KeyFrame* pKF, int N) { return N > 0 ? query(pKF, N, 0) : std::vector<KeyFrame*>(); }
    std::vector<KeyFrame*> GetCovisiblesByWeight(KeyFrame* pKF, int w) { return w > 0 ? query(pKF, 0, w) : query(pKF, 0, 1); }       // (every counted weight is at least 1)
    int GetWeight(KeyFrame* pKF, KeyFrame* pOther) { int w = 0; check(corb_covis_weight(h_, Slot(pKF), Slot(pOther), &w), "corb_covis_weight"); return w; }
    std::vector<Culling> KeyFrameCulling(KeyFrame* pCurrent, bool bMonocular, float thDepth)
    {
        std::vector<int32_t> s(cap()), nm(cap()), nr(cap()); std::vector<uint8_t> c(cap()); int n = 0;
        check(corb_covis_keyframe_culling(h_, Slot(pCurrent), bMonocular ? 1 : 0, thDepth, s.data(), nm.data(), nr.data(), c.data(), (int)cap(), &n), "corb_covis_keyframe_culling");
        std::vector<Culling> out;
        for (int i = 0; i < n; i++) out.push_back(Culling{at(s[i]), nm[i], nr[i], c[i] != 0});
        return out;
    }
    // lLocalKeyFrames, lFixedCameras, lLocalMapPoints as slots; maxKeyFrames / maxMapPoints bound the window (CORB_ERR_CAPACITY beyond)
    void LocalWindow(KeyFrame* pKF, std::vector<int32_t>& localKfSlots, std::vector<int32_t>& fixedKfSlots, std::vector<int32_t>& mpSlots, int maxKeyFrames, int maxMapPoints)
    {
        std::vector<int32_t> ks((size_t)std::max(maxKeyFrames, 1)), ms((size_t)std::max(maxMapPoints, 1)); int nl = 0, nk = 0, nm = 0;
        check(corb_covis_local_window(h_, Slot(pKF), ks.data(), maxKeyFrames, &nl, &nk, ms.data(), maxMapPoints, &nm), "corb_covis_local_window");
        localKfSlots.assign(ks.begin(), ks.begin() + nl); fixedKfSlots.assign(ks.begin() + nl, ks.begin() + nk); mpSlots.assign(ms.begin(), ms.begin() + nm);
    }
    // ---- the spanning tree ----
    void AddChild(KeyFrame* pKF, KeyFrame* pChild) { check(corb_covis_add_child(h_, Slot(pKF), Slot(pChild)), "corb_covis_add_child"); }
    void EraseChild(KeyFrame* pKF, KeyFrame* pChild) { check(corb_covis_erase_child(h_, Slot(pKF), Slot(pChild)), "corb_covis_erase_child"); }
    void ChangeParent(KeyFrame* pKF, KeyFrame* pParent) { check(corb_covis_change_parent(h_, Slot(pKF), Slot(pParent)), "corb_covis_change_parent"); }
    // mpParent's id (CORB_NO_MAP_POINT: none), mbFirstConnection and mspChildrens' ids in ascending order: what OptimizeEssentialGraph's tree edges are flattened from
    void GetTree(KeyFrame* pKF, uint64_t* parentId, bool* firstConnection, std::vector<uint64_t>* childIds)
    {
        std::vector<uint64_t> c(cap()); uint64_t p = CORB_NO_MAP_POINT; int f = 0, n = 0;
        check(corb_covis_get_tree(h_, Slot(pKF), &p, &f, c.data(), (int)cap(), &n), "corb_covis_get_tree");
        if (parentId) *parentId = p;
        if (firstConnection) *firstConnection = f != 0;
        if (childIds) childIds->assign(c.begin(), c.begin() + n);
    }
    void SetTree(KeyFrame* pKF, uint64_t parentId, bool firstConnection, const std::vector<uint64_t>& childIds)
    {
        check(corb_covis_set_tree(h_, Slot(pKF), parentId, firstConnection ? 1 : 0, childIds.data(), (int)childIds.size()), "corb_covis_set_tree");
    }
    KeyFrame* GetParent(KeyFrame* pKF) { uint64_t p; GetTree(pKF, &p, nullptr, nullptr); return byId(p); }              // getKeyFrameInCache(): NULL for a keyframe without a slot
    std::vector<KeyFrame*> GetChilds(KeyFrame* pKF)                                                                       // ascending mnId; the ones without a slot dropped (:523-532)
    {
        std::vector<uint64_t> c; GetTree(pKF, nullptr, nullptr, &c);
        std::vector<KeyFrame*> out; for (uint64_t id : c) if (KeyFrame* p = byId(id)) out.push_back(p);
        return out;
    }
    bool hasChild(KeyFrame* pKF, KeyFrame* pChild) { std::vector<uint64_t> c; GetTree(pKF, nullptr, nullptr, &c); return std::binary_search(c.begin(), c.end(), (uint64_t)pChild->mnId); }
    // the tree part of KeyFrame::SetBadFlag (:607-668), after EraseConnections(pKF); returns whether the reference sets mbBad (its `if` of :658)
    bool ReparentChildren(KeyFrame* pKF, int* nChanged = nullptr)
    {
        int n = 0, bad = 0;
        check(corb_covis_reparent_children(h_, Slot(pKF), &n, &bad), "corb_covis_reparent_children");
        if (nChanged) *nChanged = n;
        return bad != 0;
    }
    // void Tracking::UpdateLocalMap() for the frame in `slot` of `frames`: mvpLocalKeyFrames (in and out), the local points as slots and ids, *ppReferenceKF = pKFmax
    // when there is one (mpReferenceKF stays otherwise)
    adapt::LocalMapSlots UpdateLocalMap(CorbKfStore* frames, int slot, std::vector<KeyFrame*>& vpLocalKeyFrames, KeyFrame** ppReferenceKF, int maxMapPoints, int maxKeyFrames = 128)
    {
        std::vector<int32_t> prev; for (KeyFrame* p : vpLocalKeyFrames) prev.push_back(Slot(p));
        adapt::LocalMapSlots r = adapt::UpdateLocalMapSlots(h_, frames, slot, prev, std::max(maxKeyFrames, (int)prev.size()), maxMapPoints);
        vpLocalKeyFrames.clear(); for (int32_t s : r.kfSlots) vpLocalKeyFrames.push_back(at(s));
        if (ppReferenceKF && r.refSlot >= 0) *ppReferenceKF = at(r.refSlot);
        return r;
    }
    // ---- a loop event on records (corb_loop_correct_store, corb_gba_propagate_store) ----
    // vpMP[m] is the object of map-point slot first + m of the graph's map-point store; every keyframe involved is bound.  MapPoint needs one setter the reference
    // does not have, next to the two getters the tracking calls ask for: SetNormalAndDistances(normal, mfMinDistance, mfMaxDistance); KeyFrame::mTcwBefGBA is public.
    //
    // CorrectLoop's propagation (GlobalOptimize.cpp:253-338 = LoopClosing.cc:436-522) for mpCurrentKF and mg2oScw (8 doubles: quaternion x y z w, t, s); scaleFactor =
    // mpCurrentKF->mfScaleFactor (0: no UpdateNormalAndDepth).  Returns mvpCurrentConnectedKFs in the walk's order (ascending mnId), fills CorrectedSim3 /
    // NonCorrectedSim3 through makeSim3(const double* v8) and leaves in the objects what the reference leaves: SetPose + addUpdateKeyframe for every member,
    // SetWorldPos + addUpdateMapPoint + mnCorrectedByKF + mnCorrectedReference (+ normal and distances) for every corrected point, then UpdateConnections per member (:337)
    template <class MapPoint, class Mat, class Cache, class PoseMap, class MakeSim3>
    std::vector<KeyFrame*> CorrectLoop(KeyFrame* pCurrentKF, const double* Scw, float scaleFactor, CorbKfStore* kfs, CorbMpStore* mps, int first, const std::vector<MapPoint*>& vpMP,
                                       Cache* pCacher, PoseMap& CorrectedSim3, PoseMap& NonCorrectedSim3, MakeSim3 makeSim3, int* pnPointsCorrected = nullptr)
    {
        const int c = (int)cap() + 1;
        std::vector<int32_t> s((size_t)c); std::vector<double> co((size_t)c * 8), nc((size_t)c * 8); int n = 0, np = 0;
        check(corb_loop_correct_store(h_, Slot(pCurrentKF), Scw, scaleFactor, s.data(), co.data(), nc.data(), c, &n, &np), "corb_loop_correct_store");
        std::vector<KeyFrame*> connected;
        for (int i = 0; i < n; i++) {
            KeyFrame* pKFi = at(s[i]); connected.push_back(pKFi);
            CorrectedSim3[pKFi] = makeSim3(&co[(size_t)i * 8]); NonCorrectedSim3[pKFi] = makeSim3(&nc[(size_t)i * 8]);
            CorbKeyFrameMeta m; check(corb_kf_store_get_meta(kfs, s[i], &m), "corb_kf_store_get_meta");
            pKFi->SetPose(adapt::MatFactory<Mat>::from_floats(4, 4, m.Tcw)); pCacher->addUpdateKeyframe(pKFi);                                     // :332-334
        }
        std::vector<CorbMapPointRecord> rec(vpMP.size()); std::vector<CorbMapPointScratch> sc(vpMP.size());
        if (!vpMP.empty()) {
            check(corb_mp_store_get(mps, first, (int)vpMP.size(), rec.data(), nullptr, nullptr), "corb_mp_store_get");
            check(corb_mp_store_get_scratch(mps, first, (int)sc.size(), sc.data()), "corb_mp_store_get_scratch");
        }
        for (size_t m = 0; m < vpMP.size(); m++) {
            MapPoint* pMP = vpMP[m];
            if (!pMP || sc[m].corrected_by_kf != (uint64_t)pCurrentKF->mnId || pMP->mnCorrectedByKF == pCurrentKF->mnId) continue;               // corrected by THIS call
            pMP->SetWorldPos(adapt::MatFactory<Mat>::from_floats(3, 1, rec[m].world_pos)); pCacher->addUpdateMapPoint(pMP);                       // :315-316
            pMP->mnCorrectedByKF = (long unsigned int)sc[m].corrected_by_kf; pMP->mnCorrectedReference = (long unsigned int)sc[m].corrected_reference;
            if (scaleFactor > 0.f) pMP->SetNormalAndDistances(adapt::MatFactory<Mat>::from_floats(3, 1, rec[m].normal), rec[m].min_distance, rec[m].max_distance);   // :320
        }
        for (KeyFrame* pKFi : connected) UpdateConnections(pKFi);                                                                               // :337
        if (pnPointsCorrected) *pnPointsCorrected = np;
        return connected;
    }
    // the map update of RunGlobalBundleAdjustment (GlobalOptimize.cpp:463-532 = LoopClosing.cc:684-753) for mvpKeyFrameOrigins and nLoopKF.  The objects receive what
    // the reference leaves: mTcwBefGBA, SetPose, mTcwGBA and mnBAGlobalForKF + addUpdateKeyframe for every keyframe the walk reaches (the closure of the origins over
    // GetChilds(), one small read per keyframe), SetWorldPos + addUpdateMapPoint for every point it sets or moves
    template <class MapPoint, class Mat, class Cache>
    CorbGbaPropagation PropagateGlobalBA(const std::vector<KeyFrame*>& vpKeyFrameOrigins, unsigned long nLoopKF, CorbKfStore* kfs, CorbMpStore* mps, int first,
                                         const std::vector<MapPoint*>& vpMP, Cache* pCacher, int queueCap = 0)
    {
        std::vector<int32_t> origins; for (KeyFrame* p : vpKeyFrameOrigins) origins.push_back(Slot(p));
        CorbGbaPropagation r{};
        check(corb_gba_propagate_store(h_, origins.data(), (int)origins.size(), (uint64_t)nLoopKF, queueCap, &r), "corb_gba_propagate_store");
        std::vector<KeyFrame*> reached(vpKeyFrameOrigins); std::map<KeyFrame*, bool> seen;
        for (KeyFrame* p : reached) seen[p] = true;
        for (size_t i = 0; i < reached.size(); i++) for (KeyFrame* ch : GetChilds(reached[i])) if (!seen[ch]) { seen[ch] = true; reached.push_back(ch); }
        for (KeyFrame* pKF : reached) {
            const int slot = Slot(pKF); float bef[16];
            CorbKeyFrameMeta m; check(corb_kf_store_get_meta(kfs, slot, &m), "corb_kf_store_get_meta");
            check(corb_covis_get_pose_before_gba(h_, slot, bef), "corb_covis_get_pose_before_gba");
            pKF->mTcwGBA = adapt::MatFactory<Mat>::from_floats(4, 4, m.TcwGBA);                                                                    // :477
            if (m.ba_global_for_kf == (uint64_t)nLoopKF) pKF->mnBAGlobalForKF = nLoopKF;                                                         // :478
            pKF->mTcwBefGBA = adapt::MatFactory<Mat>::from_floats(4, 4, bef); pKF->SetPose(adapt::MatFactory<Mat>::from_floats(4, 4, m.Tcw));     // :484-485
            pCacher->addUpdateKeyframe(pKF);
        }
        std::vector<CorbMapPointRecord> rec(vpMP.size());
        if (!vpMP.empty()) check(corb_mp_store_get(mps, first, (int)vpMP.size(), rec.data(), nullptr, nullptr), "corb_mp_store_get");
        for (size_t m = 0; m < vpMP.size(); m++) {
            MapPoint* pMP = vpMP[m];
            if (!pMP || pMP->isBad()) continue;                                                                                                  // :498
            if (pMP->mnBAGlobalForKF != nLoopKF) {                                                                                               // :507-515
                KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
                if (!pRefKF || slot_.find(pRefKF) == slot_.end() || pRefKF->mnBAGlobalForKF != nLoopKF) continue;
            }
            pMP->SetWorldPos(adapt::MatFactory<Mat>::from_floats(3, 1, rec[m].world_pos)); pCacher->addUpdateMapPoint(pMP);                       // :504-505, :527-528
        }
        return r;
    }
    // ---- the loop edges and the essential graph on records (include/corb_essential_graph.h) ----
    void AddLoopEdge(KeyFrame* pKF, KeyFrame* pOther) { check(corb_covis_add_loop_edge(h_, Slot(pKF), Slot(pOther)), "corb_covis_add_loop_edge"); }      // KeyFrame.cc:545-550
    std::set<KeyFrame*> GetLoopEdges(KeyFrame* pKF)                                                                       // the ones without a slot dropped (:552-561)
    {
        uint64_t ids[CORB_COVIS_MAX_LOOP_EDGES]; int n = 0;
        check(corb_covis_get_loop_edges(h_, Slot(pKF), ids, CORB_COVIS_MAX_LOOP_EDGES, &n), "corb_covis_get_loop_edges");
        std::set<KeyFrame*> out; for (int i = 0; i < n; i++) if (KeyFrame* p = byId(ids[i])) out.insert(p);
        return out;
    }
    // void Optimizer::OptimizeEssentialGraph(pCache, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale) (Optimizer.cc:840-1117) through
    // corb_essential_graph_store.  The two pose maps are read through toV8(const Sim3&, double* v8) (quaternion x y z w, t, s: what CorrectLoop's makeSim3 was given);
    // a key of LoopConnections or a member of a set without a slot is a caller's error.  scaleFactor = mfScaleFactor (0: no UpdateNormalAndDepth); vpMP[m] is the
    // object of map-point slot first + m.  The objects receive what :1074-1112 leave: SetPose + addUpdateKeyframe for every keyframe with a vertex that is not
    // getFixed(), SetWorldPos + addUpdateMapPoint (+ normal and distances) for every point the call moved -- the points that are neither bad nor fixed and whose
    // nIDr (:1087-1098) names a bound keyframe that is not bad.
    template <class MapPoint, class Mat, class Cache, class PoseMap, class ToV8>
    CorbEssentialGraphResult OptimizeEssentialGraph(KeyFrame* pLoopKF, KeyFrame* pCurKF, const PoseMap& NonCorrectedSim3, const PoseMap& CorrectedSim3,
                                                    const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections, bool bFixScale, float scaleFactor, CorbKfStore* kfs,
                                                    CorbMpStore* mps, int first, const std::vector<MapPoint*>& vpMP, Cache* pCacher, ToV8 toV8, int minFeat = 100, int nIterations = 20)
    {
        std::vector<int32_t> corrSlots, lcKf, lcOff(1, 0), lcSlots; std::vector<double> co, nc;
        for (const auto& e : CorrectedSim3) {
            const auto non = NonCorrectedSim3.find(e.first);
            if (non == NonCorrectedSim3.end()) throw Error(CORB_ERR_ARG, "OptimizeEssentialGraph: CorrectedSim3 and NonCorrectedSim3 have different keys");
            corrSlots.push_back(Slot(e.first)); co.resize(co.size() + 8); nc.resize(nc.size() + 8);
            toV8(e.second, &co[co.size() - 8]); toV8(non->second, &nc[nc.size() - 8]);
        }
        for (const auto& e : LoopConnections) {
            lcKf.push_back(Slot(e.first));
            for (KeyFrame* p : e.second) lcSlots.push_back(Slot(p));
            lcOff.push_back((int32_t)lcSlots.size());
        }
        CorbEssentialGraphInput in{};
        in.loop_slot = Slot(pLoopKF); in.cur_slot = Slot(pCurKF); in.n_corr = (int32_t)corrSlots.size(); in.n_lc = (int32_t)lcKf.size();
        in.corr_slots = corrSlots.data(); in.corrected = co.data(); in.non_corrected = nc.data();
        in.lc_kf = lcKf.data(); in.lc_offset = lcOff.data(); in.lc_slots = lcSlots.data(); in.min_weight = minFeat;
        CorbEssentialGraphResult r{};
        check(corb_essential_graph_store(h_, &in, nIterations, bFixScale ? 1 : 0, scaleFactor, nullptr, nullptr, 0, &r), "corb_essential_graph_store");
        for (size_t s = 0; s < kf_.size(); s++) {                                                                                                 // :1053-1076
            KeyFrame* pKFi = kf_[s];
            if (!pKFi || pKFi->isBad() || pKFi->getFixed()) continue;
            CorbKeyFrameMeta m; check(corb_kf_store_get_meta(kfs, (int)s, &m), "corb_kf_store_get_meta");
            pKFi->SetPose(adapt::MatFactory<Mat>::from_floats(4, 4, m.Tcw)); pCacher->addUpdateKeyframe(pKFi);
        }
        std::vector<CorbMapPointRecord> rec(vpMP.size());
        if (!vpMP.empty()) check(corb_mp_store_get(mps, first, (int)vpMP.size(), rec.data(), nullptr, nullptr), "corb_mp_store_get");
        for (size_t m = 0; m < vpMP.size(); m++) {                                                                                                // :1079-1115
            MapPoint* pMP = vpMP[m];
            if (!pMP || pMP->isBad() || pMP->getFixed()) continue;
            KeyFrame* pRef = nullptr;
            if (pMP->mnCorrectedByKF == pCurKF->mnId) pRef = byId((uint64_t)pMP->mnCorrectedReference);
            else if (KeyFrame* p = pMP->GetReferenceKeyFrame()) pRef = slot_.find(p) != slot_.end() ? p : nullptr;
            if (!pRef || pRef->isBad()) continue;
            pMP->SetWorldPos(adapt::MatFactory<Mat>::from_floats(3, 1, rec[m].world_pos)); pCacher->addUpdateMapPoint(pMP);                       // :1109-1111
            if (scaleFactor > 0.f) pMP->SetNormalAndDistances(adapt::MatFactory<Mat>::from_floats(3, 1, rec[m].normal), rec[m].min_distance, rec[m].max_distance);   // :1112
        }
        return r;
    }
    KeyFrame* at(int slot) const { return slot >= 0 && slot < (int)kf_.size() ? kf_[slot] : nullptr; }
    CorbCovis* handle() const { return h_; }
private:
    KeyFrame* byId(uint64_t id) const { if (id != CORB_NO_MAP_POINT) for (KeyFrame* p : kf_) if (p && (uint64_t)p->mnId == id) return p; return nullptr; }
    size_t cap() const { return 1024; }                           // (COVIS_MAX_CONNECTIONS: no row is longer)
    std::vector<KeyFrame*> query(KeyFrame* pKF, int N, int w)
    {
        std::vector<int32_t> s(cap()); int n = 0;
        check(corb_covis_query(h_, Slot(pKF), N, w, s.data(), nullptr, (int)cap(), &n), "corb_covis_query");
        std::vector<KeyFrame*> out; for (int i = 0; i < n; i++) out.push_back(at(s[i]));
        return out;
    }
    CorbCovis* h_ = nullptr; Db* db_;
    std::map<KeyFrame*, int> slot_; std::vector<KeyFrame*> kf_;
};
}  // namespace corb

#if defined(__has_include)
#if __has_include(<opencv2/core/core.hpp>) && __has_include("KeyFrame.h") && __has_include("Frame.h") && __has_include("MapPoint.h") && __has_include("Cache.h")
#include <opencv2/core/core.hpp>
#include "KeyFrame.h"
#include "Frame.h"
#include "MapPoint.h"
#include "Cache.h"
namespace corb { namespace adapt {
template <> struct MatFactory<cv::Mat> { static cv::Mat from_floats(int rows, int cols, const float* p) { return cv::Mat(rows, cols, CV_32F, const_cast<float*>(p)).clone(); } };
} }
namespace ORB_SLAM2 {
namespace accel {
using ORBmatcher = corb::adapt::ORBmatcherT<KeyFrame, Frame, MapPoint, cv::Mat>;
using Optimizer = corb::adapt::OptimizerT<KeyFrame, Frame, MapPoint, Cache, cv::Mat>;
using MapStore = corb::adapt::MapStoreT<KeyFrame, MapPoint, cv::Mat>;
using KeyFrameInsert = corb::adapt::KeyFrameInsertT<KeyFrame, MapPoint>;
using MapPublish = corb::adapt::MapPublishT<cv::Mat>;
using FrameStore = corb::adapt::FrameStoreT<Frame, MapPoint, cv::Mat>;
using Sim3Solver = corb::Sim3Solver<KeyFrame, MapPoint>;
using PnPsolver = corb::PnPsolver<Frame, KeyFrame, MapPoint>;
using Initializer = corb::Initializer<Frame>;
using ORBVocabulary = corb::ORBVocabulary;
using KeyFrameDatabase = corb::KeyFrameDatabase<KeyFrame, Frame>;
using MapFusionDetect = corb::adapt::MapFusionDetectT<KeyFrame, corb::KeyFrameDatabase<KeyFrame, Frame>>;
using LoopDetect = corb::adapt::LoopDetectT<KeyFrame, corb::KeyFrameDatabase<KeyFrame, Frame>>;
using Covisibility = corb::Covisibility<KeyFrame, corb::KeyFrameDatabase<KeyFrame, Frame>>;
}  // namespace accel
}  // namespace ORB_SLAM2
#endif
#endif
