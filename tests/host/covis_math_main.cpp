// covis_math_main.cpp -- csrc/covis_math.h on the host: reads one case per line, writes one answer per line (tests/test_covis_math_host.py compares them with
// tests/covis_reference.py).  Floats travel as IEEE bit patterns.
//   B wa ida wb idb        covis_before
//   P w id best_w best_id  covis_pick_better
//   O in_store u_right     covis_obs_weight
//   C octave_other octave  covis_octave_counts
//   D monocular depth th   covis_depth_skipped
//   K n_redundant n_mps    covis_cull
//   L n (w id) x n         the list in covis_before order, then the pick of a walk in the order given (-1 if no weight is above 0)
#include "covis_math.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

static float bits(unsigned int u) { float f; memcpy(&f, &u, 4); return f; }

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: covis_math_main in.txt out.txt\n"); return 2; }
    FILE* in = fopen(argv[1], "r"); FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    char op;
    while (fscanf(in, " %c", &op) == 1) {
        if (op == 'B' || op == 'P') {
            int wa, wb; unsigned long long ia, ib;
            if (fscanf(in, "%d %llu %d %llu", &wa, &ia, &wb, &ib) != 4) return 3;
            fprintf(out, "%d\n", op == 'B' ? (int)covis_before(wa, ia, wb, ib) : (int)covis_pick_better(wa, ia, wb, ib));
        } else if (op == 'O') {
            int in_store; unsigned int u;
            if (fscanf(in, "%d %u", &in_store, &u) != 2) return 3;
            fprintf(out, "%d\n", covis_obs_weight(in_store != 0, bits(u)));
        } else if (op == 'C' || op == 'K') {
            int a, b;
            if (fscanf(in, "%d %d", &a, &b) != 2) return 3;
            fprintf(out, "%d\n", op == 'C' ? (int)covis_octave_counts(a, b) : (int)covis_cull(a, b));
        } else if (op == 'D') {
            int mono; unsigned int d, t;
            if (fscanf(in, "%d %u %u", &mono, &d, &t) != 3) return 3;
            fprintf(out, "%d\n", (int)covis_depth_skipped(mono, bits(d), bits(t)));
        } else if (op == 'L') {
            int n;
            if (fscanf(in, "%d", &n) != 1 || n < 0) return 3;
            std::vector<std::pair<int, unsigned long long>> v((size_t)n);
            for (auto& e : v) if (fscanf(in, "%d %llu", &e.first, &e.second) != 2) return 3;
            int bw = 0; unsigned long long bid = 0; bool any = false;
            for (const auto& e : v) if (covis_pick_better(e.first, e.second, bw, bid)) { bw = e.first; bid = e.second; any = true; }
            std::sort(v.begin(), v.end(), [](const std::pair<int, unsigned long long>& a, const std::pair<int, unsigned long long>& b) { return covis_before(a.first, a.second, b.first, b.second); });
            for (const auto& e : v) fprintf(out, "%llu:%d ", e.second, e.first);
            if (any) fprintf(out, "| %llu\n", bid); else fprintf(out, "| -1\n");
        } else return 3;
    }
    fclose(in); fclose(out);
    return 0;
}
