// trackframe_main.cpp -- drives the mirrors of include/corb_track_frame.h in corb_host.hpp (corb::TrackInitialPose, CleanVOMatches, TrackFrameFinish): one tracked
// frame against a last frame, a reference keyframe and a map filed in the stores.  TEST INFRASTRUCTURE, not product code.
//   trackframe_main <in.bin> : int32 F, n_mp, O, sensor, n_ref, n_last, n_cur, has_velocity; uint64 frame_id, last_reloc_frame_id; the map points (CorbMapPointRecord[n_mp],
//       obs_off i32[n_mp + 1], obs_kf u64[], obs_idx u32[]); three records, reference keyframe / last frame / current frame, each CorbKeyFrameMeta, CorbKeyPoint[n],
//       desc u8[n][32], u_right f32[n], mp_id u64[n]; velocity f32[16], Tlr f32[16]; the camera (fx, fy, cx, cy, bf, mb, mnMinX, mnMaxX, mnMinY, mnMaxY, 8 scale factors)
// Prints the reference's bool with the counts, the pose's bits, the frame's ids after both finish stages and Tcr's bits.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "corb_host.hpp"

namespace {
struct Record { CorbKeyFrameMeta meta; std::vector<CorbKeyPoint> kp; std::vector<uint8_t> desc; std::vector<float> ur; std::vector<uint64_t> ids; };
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    int32_t hdr[8]; uint64_t fid[2]; rd(hdr, sizeof(hdr)); rd(fid, sizeof(fid));
    const int F = hdr[0], n_mp = hdr[1], O = hdr[2], sensor = hdr[3];
    std::vector<CorbMapPointRecord> rec((size_t)n_mp); std::vector<int32_t> ooff((size_t)n_mp + 1);
    rd(rec.data(), rec.size() * sizeof(CorbMapPointRecord)); rd(ooff.data(), ooff.size() * 4);
    std::vector<uint64_t> okf((size_t)ooff[n_mp]); std::vector<uint32_t> oidx((size_t)ooff[n_mp]);
    rd(okf.data(), okf.size() * 8); rd(oidx.data(), oidx.size() * 4);
    Record r[3];
    for (int k = 0; k < 3; k++) {
        const size_t n = (size_t)hdr[4 + k];
        r[k].kp.resize(n); r[k].desc.resize(n * 32); r[k].ur.resize(n); r[k].ids.resize(n);
        rd(&r[k].meta, sizeof(CorbKeyFrameMeta)); rd(r[k].kp.data(), n * sizeof(CorbKeyPoint)); rd(r[k].desc.data(), n * 32); rd(r[k].ur.data(), n * 4); rd(r[k].ids.data(), n * 8);
    }
    float velocity[16], Tlr[16], camv[18];
    rd(velocity, sizeof(velocity)); rd(Tlr, sizeof(Tlr)); rd(camv, sizeof(camv));
    fclose(f);

    corb::check_abi();
    CorbKfStore* kfs = nullptr; CorbKfStore* frs = nullptr; CorbMpStore* mps = nullptr;
    corb::check(corb_kf_store_create(0, 1, F, &kfs), "corb_kf_store_create"); corb::check(corb_kf_store_create(0, 2, F, &frs), "corb_kf_store_create");
    corb::check(corb_mp_store_create(0, n_mp, O, &mps), "corb_mp_store_create");
    corb::check(corb_mp_store_put_host(mps, 0, n_mp, rec.data(), ooff.data(), okf.data(), oidx.data()), "corb_mp_store_put_host");
    corb::check(corb_mp_store_build_index(mps, 0, n_mp), "corb_mp_store_build_index");
    CorbKfStore* where[3] = {kfs, frs, frs}; const int slot[3] = {0, 0, 1};
    for (int k = 0; k < 3; k++) {
        corb::check(corb_kf_store_put_frame(where[k], slot[k], r[k].kp.data(), r[k].desc.data(), r[k].ur.data(), nullptr, (int)r[k].kp.size(), &r[k].meta), "corb_kf_store_put_frame");
        corb::check(corb_kf_store_set_map_points(where[k], slot[k], r[k].ids.data()), "corb_kf_store_set_map_points");
    }
    CorbTrackCamera cam;
    cam.fx = camv[0]; cam.fy = camv[1]; cam.cx = camv[2]; cam.cy = camv[3]; cam.bf = camv[4]; cam.mb = camv[5];
    cam.min_x = camv[6]; cam.max_x = camv[7]; cam.min_y = camv[8]; cam.max_y = camv[9]; cam.nlevels = 8;
    for (int l = 0; l < 16; l++) cam.scale[l] = l < 8 ? camv[10 + l] : 0.f;

    bool motion = false;
    const corb::TrackFrameOutput o = corb::TrackInitialPose(frs, 1, 0, kfs, 0, mps, cam, hdr[7] ? velocity : nullptr, Tlr, nullptr, fid[0], fid[1], sensor, &motion);
    const CorbTrackFrameResult& R = o.result;
    int n_out = 0; for (uint8_t b : o.outlier) n_out += b;
    printf("R %d %d %d %d %d %d %d %d %d %d\n", R.ok, motion ? 1 : 0, R.n_matches_first, R.searched_wide, R.n_matches, R.n_pose_inliers, R.n_matches_kept, R.n_matches_map, R.vo, n_out);
    printf("T"); for (int i = 0; i < 16; i++) { uint32_t u; memcpy(&u, &R.Tcw[i], 4); printf(" %08x", u); } printf("\n");
    float Tcr[16];
    corb::CleanVOMatches(frs, 1, kfs, 0, mps);
    corb::TrackFrameFinish(frs, 1, kfs, 0, mps, Tcr);
    std::vector<uint64_t> ids(r[2].kp.size() + 1);
    corb::check(corb_kf_store_get_map_points(frs, 1, ids.data(), (int)r[2].kp.size()), "corb_kf_store_get_map_points");
    printf("I"); for (size_t i = 0; i < r[2].kp.size(); i++) printf(" %llu", (unsigned long long)ids[i]); printf("\n");
    printf("C"); for (int i = 0; i < 16; i++) { uint32_t u; memcpy(&u, &Tcr[i], 4); printf(" %08x", u); } printf("\n");
    corb_kf_store_destroy(kfs); corb_kf_store_destroy(frs); corb_mp_store_destroy(mps);
    return R.ok ? 0 : 1;
}
