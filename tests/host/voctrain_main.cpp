// voctrain_main.cpp -- csrc/voctrain_math.h compiled for the host (-ffp-contract=off): reads training cases from a binary file, trains each level by level and prints the
// flat vocabulary and the statistics as integers and IEEE bit patterns in hex.  tests/test_voctrain_math_host.py holds the output byte-equal to the recursive definition
// tests/voctrain_reference.py.  Stand-alone (no GPU, no library): the place for a sanitizer build (g++ -fsanitize=address,undefined).
//   file: i32 n_cases | per case: i32 k, L, max_iterations, n_images | u64 seed | offset[n_images + 1] i32 | desc[offset[n_images]][32]
//   out : per case `C n_nodes` p l d w s ln li, or `E message`; with digits >= 0 as a fourth argument the text form (vt_text) of the last case goes to a fifth
#include "voctrain_math.h"
#include <cstdlib>

#ifdef VT_HOST_SHARED
// the same serial code as a shared object, so that a measuring process can run it in-process (tools/voc_train_rate.py): g++ -O3 -shared -fPIC -DVT_HOST_SHARED
extern "C" int vt_host_train(const uint8_t* desc, const int32_t* offset, int n_images, int k, int L, unsigned long long seed, int max_iterations,
                             int32_t* parent, int32_t* is_leaf, uint8_t* descriptor, double* weight, int cap_nodes, int* n_nodes)
{
    const size_t N = (size_t)offset[n_images];
    std::vector<unsigned long long> d(N * VT_WORDS + 1); memcpy(d.data(), desc, N * 32);
    VtFlat f; VtStats st; BowVocHost words;
    if (!vt_train_host(d.data(), offset, n_images, k, L, seed, max_iterations, &f, &st, &words).empty()) return 1;
    *n_nodes = (int)f.parent.size();
    if (*n_nodes > cap_nodes) return 2;
    std::copy(f.parent.begin(), f.parent.end(), parent); std::copy(f.is_leaf.begin(), f.is_leaf.end(), is_leaf);
    std::copy(f.descriptor.begin(), f.descriptor.end(), descriptor); std::copy(f.weight.begin(), f.weight.end(), weight);
    return 0;
}
#else
static std::vector<char> buf; static size_t at = 0;
template <class T> static T rd() { T v; if (at + sizeof(T) > buf.size()) { fprintf(stderr, "truncated case file\n"); exit(2); } memcpy(&v, &buf[at], sizeof(T)); at += sizeof(T); return v; }
template <class T> static std::vector<T> rdv(size_t n) { std::vector<T> v(n); if (at + n * sizeof(T) > buf.size()) { fprintf(stderr, "truncated case file\n"); exit(2); } if (n) memcpy(v.data(), &buf[at], n * sizeof(T)); at += n * sizeof(T); return v; }
static unsigned long long bits(double v) { unsigned long long b; memcpy(&b, &v, 8); return b; }

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: voctrain_main cases.bin out.txt [digits text.txt]\n"); return 1; }
    { std::ifstream f(argv[1], std::ios::binary); if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; } buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
    FILE* o = fopen(argv[2], "w"); if (!o) return 1;
    const int n_cases = rd<int32_t>();
    VtFlat f; int k = 0, L = 0;
    for (int c = 0; c < n_cases; c++) {
        k = rd<int32_t>(); L = rd<int32_t>(); const int max_it = rd<int32_t>(), n_images = rd<int32_t>(); const unsigned long long seed = rd<uint64_t>();
        if (n_images < 0) return 2;
        const auto offset = rdv<int32_t>((size_t)n_images + 1);
        for (int i = 0; i < n_images; i++) if (offset[i + 1] < offset[i] || offset[0] != 0) return 2;
        const size_t N = (size_t)offset[n_images];
        const auto bytes = rdv<uint8_t>(N * 32);
        std::vector<unsigned long long> d(N * VT_WORDS + 1); if (N) memcpy(d.data(), bytes.data(), N * 32);
        VtStats st; BowVocHost words;
        const std::string err = vt_train_host(d.data(), offset.data(), n_images, k, L, seed, max_it, &f, &st, &words);
        if (!err.empty()) { fprintf(o, "E %s\n", err.c_str()); continue; }
        const size_t n = f.parent.size();
        fprintf(o, "C %zu\np", n); for (size_t i = 0; i < n; i++) fprintf(o, " %d", f.parent[i]);
        fprintf(o, "\nl"); for (size_t i = 0; i < n; i++) fprintf(o, " %d", f.is_leaf[i]);
        fprintf(o, "\nd "); for (size_t i = 0; i < n * 32; i++) fprintf(o, "%02x", f.descriptor[i]);
        fprintf(o, "\nw"); for (size_t i = 0; i < n; i++) fprintf(o, " %016llx", bits(f.weight[i]));
        fprintf(o, "\ns %d %d %d %d %d %d %d %d", st.nodes, st.words, st.kmeans_nodes, st.trivial_nodes, st.short_nodes, st.max_iterations_seen, st.capped_nodes, st.empty_cluster_events);
        fprintf(o, "\nln"); for (int i = 0; i < VT_MAX_LEVELS; i++) fprintf(o, " %d", st.level_nodes[i]);
        fprintf(o, "\nli"); for (int i = 0; i < VT_MAX_LEVELS; i++) fprintf(o, " %d", st.level_max_iterations[i]);
        fprintf(o, "\n");
    }
    fclose(o);
    if (argc > 4 && n_cases > 0) { const std::string t = vt_text(k, L, f, atoi(argv[3])); FILE* x = fopen(argv[4], "w"); if (!x) return 1; fwrite(t.data(), 1, t.size(), x); fclose(x); }
    return 0;
}
#endif
