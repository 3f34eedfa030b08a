// covis_math.h -- the rules of the covisibility graph, stated once for the kernels (covis_kernels.hip) and a stand-alone host program (tests/host/covis_math_main.cpp):
// the (weight, id) order of mvpOrderedConnectedKeyFrames (C/src/KeyFrame.cc:150-168, :471-482), the fallback pick of UpdateConnections (:450-455, :466-469), the weight
// of one observation in MapPoint::Observations() (C/src/MapPoint.cc:153-158, :250-253) and the decision of LocalMapping::KeyFrameCulling (C/src/LocalMapping.cc:645).
// tests/covis_reference.py is the definition.  Integers only, except the one double product of the culling decision.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define COVIS_HD __host__ __device__ inline
#else
#define COVIS_HD inline
#endif

#define COVIS_TH_OBS 3                       // thObs of KeyFrameCulling (LocalMapping.cc:604-605)
#define COVIS_NO_ID 0xFFFFFFFFFFFFFFFFull     // "none" (CORB_NO_MAP_POINT's value): the first parent of an empty counter, an empty table slot

// true when (wa, ida) stands before (wb, idb) in an ordered list: sort() ascends in pair<int, LightKeyFrame> (LightKeyFrame::operator< compares mnId) and the
// list is filled by push_front, so it descends in (weight, id) -- of two equal weights the higher id comes first
COVIS_HD bool covis_before(int wa, unsigned long long ida, int wb, unsigned long long idb)
{
    return wa > wb || (wa == wb && ida > idb);
}
// the walk of :450-455 ascends in the id and replaces the pick on a strict `>`: true when (w, id) takes the place of the pick (best_w, best_id) whatever the
// order the two are met in.  The walk starts from nmax = 0, so a candidate needs w > 0 -- every counted weight is.
COVIS_HD bool covis_pick_better(int w, unsigned long long id, int best_w, unsigned long long best_id)
{
    return w > best_w || (w == best_w && id < best_id);
}
// what one observation adds to nObs: 2 when the observing keyframe holds a right coordinate for the feature (MapPoint.cc:155-158), else 1; an observer the store does
// not hold counts 1 (the rule corb_local_ba_store documents)
COVIS_HD int covis_obs_weight(bool observer_in_store, float u_right)
{
    return observer_in_store && u_right >= 0.0f ? 2 : 1;
}
// `scaleLeveli <= scaleLevel + 1` (LocalMapping.cc:630)
COVIS_HD bool covis_octave_counts(int octave_other, int octave_this)
{
    return octave_other <= octave_this + 1;
}
// the depth test of the non-monocular case (:612-615): true when the feature is skipped
COVIS_HD bool covis_depth_skipped(int monocular, float depth, float th_depth)
{
    return !monocular && (depth > th_depth || depth < 0.0f);
}
// `nRedundantObservations > 0.9 * nMPs` (:645): an int against a double product
COVIS_HD bool covis_cull(int n_redundant, int n_mps)
{
    return (double)n_redundant > 0.9 * (double)n_mps;
}
