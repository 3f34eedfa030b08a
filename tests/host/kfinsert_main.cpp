// kfinsert_main.cpp -- csrc/kfinsert_math.h on the host: one request per input line, floats as IEEE bit patterns in hex, one answer line each
// (tests/test_kfinsert_math_host.py compares them with tests/kfinsert_reference.py).  usage: kfinsert_main in.txt out.txt
#include "kfinsert_math.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

static float f_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t b_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static bool floats(std::istringstream& in, float* out, int n)
{
    for (int i = 0; i < n; i++) { std::string t; if (!(in >> t)) return false; out[i] = f_of((uint32_t)std::stoul(t, nullptr, 16)); }
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: kfinsert_main in.txt out.txt\n"); return 2; }
    std::ifstream in(argv[1]); FILE* out = fopen(argv[2], "w");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line); std::string op; ls >> op;
        if (op == "V") { int m, near, mode; ls >> m >> near >> mode; fprintf(out, "V %d\n", kfi_n_visited(m, near, mode)); }
        else if (op == "C") { float v[2]; if (!floats(ls, v, 2)) return 3; fprintf(out, "C %d %d\n", kfi_is_candidate(v[0]) ? 1 : 0, kfi_is_far(v[0], v[1]) ? 1 : 0); }
        else if (op == "U") {
            float v[23]; if (!floats(ls, v, 23)) return 3;
            NpCam c; for (int k = 0; k < 12; k++) c.T[k] = v[k];
            c.fx = v[16]; c.fy = v[17]; c.cx = v[18]; c.cy = v[19]; np_cam_finish(c);
            float X[3]; np_unproject_uv(c, v[20], v[21], v[22], X);
            fprintf(out, "U %08x %08x %08x\n", b_of(X[0]), b_of(X[1]), b_of(X[2]));
        } else if (op == "S" || op == "T") {
            float T[16], X[3], scale[16], r[5]; int octave, nlevels;
            if (!floats(ls, T, 16) || !floats(ls, X, 3)) return 3;
            ls >> octave >> nlevels;
            if (!floats(ls, scale, 16)) return 3;
            if (op == "S") kfi_single_observation(T, X, octave, nlevels, scale, r);
            else { NpCam c; for (int k = 0; k < 12; k++) c.T[k] = T[k]; c.fx = c.fy = 1.f; c.cx = c.cy = 0.f; np_cam_finish(c); kfi_temporal_point(c, X, octave, nlevels, scale, r); }
            fprintf(out, "%s %08x %08x %08x %08x %08x\n", op.c_str(), b_of(r[0]), b_of(r[1]), b_of(r[2]), b_of(r[3]), b_of(r[4]));
        } else if (op == "R") { int f, v; ls >> f >> v; fprintf(out, "R %d\n", kfi_found_ratio_culls(f, v) ? 1 : 0); }
        else if (op == "W") { int at; float u[1]; ls >> at; if (!floats(ls, u, 1)) return 3; fprintf(out, "W %d\n", kfi_obs_weight(at != 0, u[0])); }
        else if (op == "D") {
            int bad, f, v, w, th; unsigned long long cur; long long first; ls >> bad >> f >> v >> cur >> first >> w >> th;
            fprintf(out, "D %d\n", kfi_cull_decision(bad != 0, f, v, cur, first, w, th));
        } else { fprintf(stderr, "unknown request '%s'\n", op.c_str()); return 3; }
    }
    fclose(out);
    return 0;
}
