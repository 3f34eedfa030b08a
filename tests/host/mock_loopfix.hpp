// mock_loopfix.hpp -- TEST DOUBLES (test infrastructure, not product code): tests/host/mock_orbslam.hpp's KeyFrame and MapPoint with the members the loop-correction
// methods of corb::Covisibility touch in addition (corbslam_client/include/KeyFrame.h:63 mTcwBefGBA; the setter INTEGRATION.md asks MapPoint.h for).
#pragma once
#include "mock_orbslam.hpp"

namespace mock {
struct LoopKeyFrame : KeyFrame { Mat mTcwBefGBA; };
struct LoopMapPoint : MapPoint {
    LoopKeyFrame* loopRef = nullptr;
    LoopKeyFrame* GetReferenceKeyFrame() { return loopRef; }
    void SetNormalAndDistances(const Mat& n, float minD, float maxD) { normal = n; minDistance = minD; maxDistance = maxD; }
};
}  // namespace mock
