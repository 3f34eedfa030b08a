// initializer_main.cpp -- csrc/init_math.h on the host: reads a file of Initializer problems, runs every step of corb_mono_initialize serially (the same text the
// kernels compile) and writes the results.  tests/test_init_math_host.py holds the output bit-equal to tests/initializer_reference.py.
//   in : int32 n_problems, max_iterations; float sigma, min_parallax; int32 min_triangulated;
//        per problem: int32 n1, n2; float fx, fy, cx, cy; n1 x (x, y) float; n2 x (x, y) float; n1 x int32 matches12;
//        then n_problems x max_iterations x 8 int32 rand_values
//   out: per problem: the 264 bytes of CorbInitResult; n1 x 3 float vP3D; n1 bytes vbTriangulated; N bytes vbMatchesInliersH; N bytes vbMatchesInliersF;
//        max_iterations x 2 float scores
// A third argument `repeats` times the serial pass and prints "seconds_per_pass <s>".
#include "init_math.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s in out [repeats]\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int P = 0, its = 0, min_tri = 0; float sigma = 0, min_par = 0;
    if (!rd(f, &P, 1) || !rd(f, &its, 1) || !rd(f, &sigma, 1) || !rd(f, &min_par, 1) || !rd(f, &min_tri, 1)) return 2;
    std::vector<InitProb> prob(P); std::vector<InitMatch> match;
    int capN = 0, cap1 = 0;
    for (int c = 0; c < P; c++) {
        int n1 = 0, n2 = 0; float K[4];
        if (!rd(f, &n1, 1) || !rd(f, &n2, 1) || !rd(f, K, 4)) return 2;
        std::vector<float> k1(2 * (size_t)n1), k2(2 * (size_t)n2); std::vector<int> m12(n1);
        if (!rd(f, k1.data(), k1.size()) || !rd(f, k2.data(), k2.size()) || !rd(f, m12.data(), m12.size())) return 2;
        InitProb& p = prob[c];
        p.n1 = n1; p.match_off = (int)match.size(); p.pad = 0; p.fx = K[0]; p.fy = K[1]; p.cx = K[2]; p.cy = K[3];
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) match.push_back({k1[2 * i], k1[2 * i + 1], k2[2 * m12[i]], k2[2 * m12[i] + 1], i, m12[i]});
        p.N = (int)match.size() - p.match_off;
        if (p.N < 8) return 3;
        init_normalize(k1.data(), 2, n1, p.nrm1); init_normalize(k2.data(), 2, n2, p.nrm2);
        if (p.N > capN) capN = p.N;
        if (n1 > cap1) cap1 = n1;
    }
    std::vector<int> rv((size_t)P * its * 8);
    if (!rd(f, rv.data(), rv.size())) return 2;
    fclose(f);

    InitDev d; memset(&d, 0, sizeof(d));
    d.n_problems = P; d.max_iterations = its; d.words = (capN + 63) / 64; d.cap1 = cap1; d.p3d_stride = cap1; d.flags_stride = capN; d.min_triangulated = min_tri;
    d.sigma = sigma; d.min_parallax = min_par; d.cos_thr_f = init_cos_threshold(min_par, true); d.cos_thr_h = init_cos_threshold(min_par, false);
    const size_t nh = (size_t)P * its * 2, nc = (size_t)P * 8;
    std::vector<float> scores(nh), hyp_m(nh * 9), cand_p3d(nc * cap1 * 3), cand_cos(nc * d.words * 64), p3d((size_t)P * cap1 * 3);
    std::vector<unsigned long long> mask(nh * d.words);
    std::vector<unsigned char> cand_good(nc * cap1), cand_pushed(nc * d.words * 64), tri((size_t)P * cap1), inl_h((size_t)P * capN), inl_f((size_t)P * capN);
    std::vector<InitSel> sel(P); std::vector<InitResult> res(P);
    d.prob = prob.data(); d.match = match.data(); d.rand_values = rv.data(); d.scores = scores.data(); d.hyp_m = hyp_m.data(); d.mask = mask.data(); d.sel = sel.data();
    d.cand_p3d = cand_p3d.data(); d.cand_good = cand_good.data(); d.cand_cos = cand_cos.data(); d.cand_pushed = cand_pushed.data();
    d.res = res.data(); d.p3d = p3d.data(); d.tri = tri.data(); d.inl_h = inl_h.data(); d.inl_f = inl_f.data();

    const int repeats = argc > 3 ? atoi(argv[3]) : 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < (repeats > 0 ? repeats : 1); r++) {
        std::fill(cand_p3d.begin(), cand_p3d.end(), 0.f); std::fill(cand_good.begin(), cand_good.end(), 0);
        std::fill(p3d.begin(), p3d.end(), 0.f); std::fill(tri.begin(), tri.end(), 0);
        memset(res.data(), 0, res.size() * sizeof(InitResult));
        init_run_serial(d);
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (repeats > 0) printf("seconds_per_pass %.9f\n", dt / repeats);

    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    for (int c = 0; c < P; c++) {
        init_fill_parallax(res[c]);
        fwrite(&res[c], sizeof(InitResult), 1, g);
        fwrite(p3d.data() + (size_t)c * cap1 * 3, 4, (size_t)prob[c].n1 * 3, g);
        fwrite(tri.data() + (size_t)c * cap1, 1, prob[c].n1, g);
        fwrite(inl_h.data() + (size_t)c * capN, 1, prob[c].N, g);
        fwrite(inl_f.data() + (size_t)c * capN, 1, prob[c].N, g);
        fwrite(scores.data() + (size_t)c * its * 2, 4, (size_t)its * 2, g);
    }
    fclose(g);
    return 0;
}
