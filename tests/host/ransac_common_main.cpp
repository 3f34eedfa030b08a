// ransac_common_main.cpp -- the plain C++ part of csrc/ransac_common.h on its own (tests/test_ransac_common_host.py): the draw rule against a literal std::vector
// emulation of the reference's loop, and draws, caps, scattered flags and the range check for a table of inputs that the Python side holds equal to
// tests/ransac_reference.py.
//   ransac_common_main check            every draw case below; ends with "<cases> draws, <mismatches> mismatches"
//   ransac_common_main table <file>     one answer line per input line:
//     draw <set size> <N> <r ...>                               -> the drawn indices
//     cap <N> <nMinInliers> <epsilon's bits> <probability> <max_iterations>   -> the cap
//     scatter <N> <stride> <words> <has index> <mask words ...> <index ...>   -> the stride flags as 0 / 1
//     rand <count> <values ...>                                 -> ok, or the message
#include "ransac_common.h"
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

static char g_error[256];
void corb_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_error, sizeof(g_error), fmt, ap); va_end(ap); }

// the reference's text: vAvailableIndices = 0 .. N-1; randi = DUtils::Random::RandomInt(0, size - 1); the pick is replaced by the back, which is popped
static std::vector<int> draw_literal(const int* r, int n, int N)
{
    std::vector<int> avail((size_t)N), out;
    for (int i = 0; i < N; i++) avail[(size_t)i] = i;
    for (int k = 0; k < n; k++) {
        const int d = (int)avail.size() - 1 - 0 + 1;
        const int randi = (int)(((double)r[k] / ((double)2147483647 + 1.0)) * d) + 0;
        out.push_back(avail.at((size_t)randi));
        avail.at((size_t)randi) = avail.back(); avail.pop_back();
    }
    return out;
}
static std::vector<int> draw_rule(const int* r, int n, int N)
{
    std::vector<int> idx((size_t)n, -1);
    if (n == 3) ransac_draw<3>(r, n, N, idx.data()); else ransac_draw<8>(r, n, N, idx.data());          // the sizes the kernels use: Sim3 3, PnP and the Initializer 8
    return idx;
}
// the smallest rand() value that RandomInt maps to position p of a vector of `size`
static int smallest_r(int p, int size)
{
    long long r = ((long long)p << 31) / size;
    while ((int)(((double)r / 2147483648.0) * size) < p) r++;
    return (int)r;
}

static long long g_cases = 0, g_mismatches = 0;
static void compare(const int* r, int n, int N, const int* want_pos)
{
    const std::vector<int> got = draw_rule(r, n, N), want = draw_literal(r, n, N);
    bool ok = got == want;
    for (int k = 0; want_pos && k < n; k++) ok = ok && (int)(((double)r[k] / 2147483648.0) * (N - k)) == want_pos[k];
    g_cases++;
    if (!ok) { if (g_mismatches++ < 10) { printf("mismatch: n %d N %d r", n, N); for (int k = 0; k < n; k++) printf(" %d", r[k]); printf("\n"); } }
}
// every tuple of positions (p_k < N - k) of a set of n, each reached by the smallest r that maps to it
static void all_positions(int n, int N)
{
    int pos[8] = {0}, r[8];
    for (;;) {
        for (int k = 0; k < n; k++) r[k] = smallest_r(pos[k], N - k);
        compare(r, n, N, pos);
        int k = n - 1;
        while (k >= 0 && ++pos[k] == N - k) pos[k--] = 0;
        if (k < 0) return;
    }
}
static int check()
{
    for (int N = 3; N <= 9; N++) all_positions(3, N);
    for (int N = 4; N <= 7; N++) all_positions(4, N);
    std::mt19937 gen(20240607u);
    for (int n = 4; n <= 8; n++)
        for (int N = n; N <= n + 3; N++)
            for (int t = 0; t < 4000; t++) {
                int r[8];
                for (int k = 0; k < n; k++) r[k] = (int)(gen() >> 1);
                compare(r, n, N, nullptr);
            }
    const int top[8] = {2147483647, 2147483647, 2147483647, 2147483647, 2147483647, 2147483647, 2147483647, 2147483647};      // the last position every time
    for (int n = 3; n <= 8; n++) compare(top, n, n, nullptr);
    printf("%lld draws, %lld mismatches\n", g_cases, g_mismatches);
    return g_mismatches ? 1 : 0;
}

static int table(const char* path)
{
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string what; in >> what;
        if (what == "draw") {
            int n, N; in >> n >> N;
            std::vector<int> r((size_t)n); for (int& v : r) in >> v;
            for (int v : draw_rule(r.data(), n, N)) printf("%d ", v);
            printf("\n");
        } else if (what == "cap") {
            int N, m, max_its; uint32_t bits; double probability; in >> N >> m >> bits >> probability >> max_its;
            float epsilon; memcpy(&epsilon, &bits, 4);
            printf("%d\n", ransac_iteration_cap(N, m, epsilon, probability, max_its));
        } else if (what == "scatter") {
            int N, stride, words, has_index; in >> N >> stride >> words >> has_index;
            std::vector<unsigned long long> mask((size_t)words); for (auto& v : mask) in >> v;
            std::vector<int> index(has_index ? (size_t)N : 0); for (int& v : index) in >> v;
            std::vector<uint8_t> flags((size_t)stride, 0);
            ransac_scatter_flags(mask.data(), N, has_index ? index.data() : nullptr, stride, flags.data());
            for (uint8_t v : flags) printf("%d", (int)v);
            printf("\n");
        } else if (what == "rand") {
            size_t count; in >> count;
            std::vector<int32_t> v(count); for (int32_t& x : v) in >> x;
            g_error[0] = 0;
            const bool ok = ransac_rand_values_ok("who", v.data(), count);
            printf("%s\n", ok ? "ok" : g_error);
        } else { printf("unknown line: %s\n", line.c_str()); return 2; }
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    if (argc == 3 && !strcmp(argv[1], "table")) return table(argv[2]);
    printf("usage: ransac_common_main check | table <file>\n");
    return 2;
}
