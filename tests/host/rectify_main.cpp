// rectify_main.cpp -- corb::StereoRectifier (corb-slam_amd/host/corb_host.hpp) compiles and links against the C-ABI alone; with a device it rectifies one small
// raw pair and prints the counts of the frame (tests/test_rectify_host.py builds it; running it needs a GPU).
#include <corb_host.hpp>
#include <cstdio>

int main()
{
    const int w = 129, h = 97, rw = 141, rh = 103;
    const std::vector<double> K{120, 0, 70, 0, 120, 51, 0, 0, 1}, D{-0.05, 0.01, 0, 0, 0}, R{1, 0, 0, 0, 1, 0, 0, 0, 1};
    const std::vector<double> Pl{110, 0, 64, 0, 0, 110, 48, 0, 0, 0, 1, 0}, Pr{110, 0, 64, -12, 0, 110, 48, 0, 0, 0, 1, 0};
    try {
        corb::StereoFrontend sf(300, 1.2f, 3, 20, 7, w, h, 110.0f, 12.0f, 1);
        corb::StereoRectifier rect(sf, K, D, R, Pl, K, D, R, Pr, rw, rh);
        std::vector<float> mx((size_t)w * h), my((size_t)w * h);
        rect.Maps(0, mx.data(), my.data());
        rect.SetMaps(1, mx.data(), my.data());
        std::vector<uint8_t> raw((size_t)2 * rw * rh);
        for (size_t i = 0; i < raw.size(); i++) raw[i] = (uint8_t)((i * 2654435761u) >> 24);
        const CorbStereoFrameLayout lay = sf.FrameLayout();
        std::vector<uint8_t> block((size_t)lay.frame_bytes);
        rect.Frames(1, raw.data(), block.data());
        const corb::StereoFrontend::FrameResult r = corb::StereoFrontend::FromBlock(lay, block.data());
        rect.UploadBatch(0, 1, raw.data()); sf.Run(1); sf.Sync();
        const corb::StereoFrontend::FrameResult q = sf.Fetch(0);
        printf("%zu %zu keypoints, map(0,0) = %g %g\n", r.mvKeys.size(), r.mvKeysRight.size(), (double)mx[0], (double)my[0]);
        return q.mvKeys.size() == r.mvKeys.size() ? 0 : 1;
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 3; }
}
