// Drives corb::RgbdFrontend (corb-slam_amd/host/corb_host.hpp) for tests/test_gpu_rgbd_host.py: one frame's input file in, the FrameResult out.
// usage: rgbd_main input.bin result.bin sensor channels rgb width height nfeatures fx fy cx cy k1 k2 p1 p2 k3 bf depth_map_factor depth_format
// result.bin: int32 n, float bounds[4], KeyPoint mvKeys[n], KeyPoint mvKeysUn[n], uint8 mDescriptors[n][32], float mvuRight[n], float mvDepth[n]
#include "corb_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 21) { fprintf(stderr, "usage: rgbd_main input.bin result.bin sensor channels rgb width height nfeatures fx fy cx cy k1 k2 p1 p2 k3 bf dmf depth_format\n"); return 2; }
    CorbCameraConfig cfg{};
    cfg.sensor = atoi(argv[3]); cfg.channels = atoi(argv[4]); cfg.rgb = atoi(argv[5]);
    cfg.orb = CorbOrbConfig{atoi(argv[8]), 1.2f, 8, 20, 7, atoi(argv[6]), atoi(argv[7]), 0, 0};
    cfg.max_frames = 1;
    float* f[] = {&cfg.fx, &cfg.fy, &cfg.cx, &cfg.cy, &cfg.k1, &cfg.k2, &cfg.p1, &cfg.p2, &cfg.k3, &cfg.bf, &cfg.depth_map_factor};
    for (int i = 0; i < 11; i++) *f[i] = (float)atof(argv[9 + i]);
    cfg.depth_format = atoi(argv[20]);
    try {
        corb::RgbdFrontend fe(cfg);
        std::vector<uint8_t> in((size_t)fe.InputBytes());
        FILE* fi = fopen(argv[1], "rb");
        if (!fi || fread(in.data(), 1, in.size(), fi) != in.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
        fclose(fi);
        const corb::RgbdFrontend::FrameResult r = fe.ProcessFrame(in.data());
        const int32_t n = (int32_t)r.mvKeys.size();
        const float b[4] = {r.mnMinX, r.mnMaxX, r.mnMinY, r.mnMaxY};
        FILE* fo = fopen(argv[2], "wb");
        if (!fo) return 1;
        fwrite(&n, 4, 1, fo); fwrite(b, 4, 4, fo);
        fwrite(r.mvKeys.data(), sizeof(corb::KeyPoint), n, fo); fwrite(r.mvKeysUn.data(), sizeof(corb::KeyPoint), n, fo);
        fwrite(r.mDescriptors.data.data(), 1, r.mDescriptors.data.size(), fo);
        fwrite(r.mvuRight.data(), 4, n, fo); fwrite(r.mvDepth.data(), 4, n, fo);
        fclose(fo);
        printf("n=%d\n", n);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
