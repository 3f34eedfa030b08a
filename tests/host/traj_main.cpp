// traj_main.cpp -- drives the mirror of include/corb_trajectory.h in corb_host.hpp (corb::Trajectory): keyframes filed in a store with their spanning tree, some of
// them culled (SetBadPose, then CORB_KF_BAD, then the poses a later optimisation left), a log of frames, and the reference's three dumps.  TEST INFRASTRUCTURE, not
// product code.
//   traj_main <in.bin> <kitti.txt> <tum.txt> <keyframes.txt> : int32 n_slots, n_kf, n_cull, n_entries, sensor, origin_slot; per keyframe int32 slot, pad,
//       CorbKeyFrameMeta, uint64 parent id, double mTimeStamp; per cull int32 slot, pad, the pose afterwards f32[16]; per entry int32 ref_slot (-1: the `else` branch),
//       lost; f32 Tcr[16]; double time
// Prints the statistics of both frame exports and the number of keyframe rows; the files hold the text.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "corb_host.hpp"

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    auto rd = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
    int32_t hdr[6]; rd(hdr, sizeof(hdr));
    const int S = hdr[0], n_kf = hdr[1], n_cull = hdr[2], n_entries = hdr[3], sensor = hdr[4], origin = hdr[5];
    corb::check_abi();
    CorbKfStore* kfs = nullptr; CorbMpStore* mps = nullptr; CorbCovis* g = nullptr;
    corb::check(corb_kf_store_create(0, S, 4, &kfs), "corb_kf_store_create");
    corb::check(corb_mp_store_create(0, 4, 4, &mps), "corb_mp_store_create");
    std::vector<int32_t> slots((size_t)n_kf); std::vector<uint64_t> parent((size_t)n_kf); std::vector<double> when((size_t)n_kf);
    for (int k = 0; k < n_kf; k++) {
        int32_t sp[2]; CorbKeyFrameMeta meta; rd(sp, sizeof(sp)); rd(&meta, sizeof(meta)); rd(&parent[k], 8); rd(&when[k], 8);
        slots[k] = sp[0];
        const int32_t off[2] = {0, 1}; CorbKeyPoint kp; std::memset(&kp, 0, sizeof(kp));
        corb::check(corb_kf_store_put_batch(kfs, sp[0], 1, &meta, off, &kp, nullptr, nullptr, nullptr, nullptr), "corb_kf_store_put_batch");
    }
    corb::check(corb_covis_create(kfs, mps, 8, &g), "corb_covis_create");
    int rc = 0;
    {
        corb::Trajectory traj(g, n_entries > 0 ? n_entries : 1, sensor);
        for (int k = 0; k < n_kf; k++) {
            corb::check(corb_covis_set_tree(g, slots[k], parent[k], 0, nullptr, 0), "corb_covis_set_tree");
            traj.SetKeyFrameTime(slots[k], when[k]);
        }
        for (int k = 0; k < n_cull; k++) {
            int32_t sp[2]; float after[16]; rd(sp, sizeof(sp)); rd(after, sizeof(after));
            traj.SetBadPose(sp[0]);
            CorbKeyFrameMeta m; corb::check(corb_kf_store_get_meta(kfs, sp[0], &m), "corb_kf_store_get_meta");
            m.flags |= CORB_KF_BAD; std::memcpy(m.Tcw, after, sizeof(after));
            corb::check(corb_kf_store_set_meta(kfs, sp[0], &m), "corb_kf_store_set_meta");
        }
        for (int k = 0; k < n_entries; k++) {
            int32_t rl[2]; float Tcr[16]; double ts; rd(rl, sizeof(rl)); rd(Tcr, sizeof(Tcr)); rd(&ts, 8);
            if (rl[0] < 0) traj.AppendLost(rl[1] != 0); else traj.Append(nullptr, 0, rl[0], Tcr, ts, rl[1] != 0);
        }
        fclose(f);
        for (int format = 0; format < 2; format++) {
            const corb::TrajectoryRows r = traj.Frames(format, origin);
            printf("%c %d %d %d %d %d %d %d\n", format == 0 ? 'K' : 'T', r.n(), r.stats.n_entries, r.stats.n_rows, r.stats.n_lost_skipped, r.stats.n_ref_gone, r.stats.n_chain_broken, r.stats.max_chain);
        }
        printf("F %d\n", traj.KeyFrames(S).n());
        const bool a = traj.SaveTrajectoryKITTI(argv[2], origin), b = traj.SaveTrajectoryTUM(argv[3], origin);
        traj.SaveKeyFrameTrajectoryTUM(argv[4]);
        printf("S %d %d %zu\n", a ? 1 : 0, b ? 1 : 0, corb::Trajectory::Format(2, traj.KeyFrames(S)).size());
        rc = (a && b) ? 0 : 1;
    }
    corb_covis_destroy(g); corb_kf_store_destroy(kfs); corb_mp_store_destroy(mps);
    return rc;
}
