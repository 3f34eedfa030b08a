// corb_voctrain.cpp -- C-ABI host side of vocabulary training and export (include/corb_voc_train.h): the level loop over csrc/voctrain_kernels.hip, the weights through
// the existing descent kernel, and a vocabulary back as flat arrays or as the reference's text.  A training call owns what it uses: device buffers from hipMalloc, freed
// before it returns, and a stream of its own -- an offline job that holds N x 32 bytes and permutations for seconds does not draw from the per-frame arenas.  Per level
// the host reads back one block of per-segment results (centres, counts, cluster sizes) and builds the next segment table from it; per pass of the multi-workgroup
// kernels it reads one flag.  Both loops are bounded by max_iterations.
#include "voctrain_internal.h"
#include "store_internal.h"
#include "store_host.h"
#include "../../include/corb_voc_train.h"
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "host_util.h"

static_assert(CORB_VOC_TRAIN_MAX_LEVELS == VT_MAX_LEVELS, "per-level statistics");

namespace {

// CORB_VOC_TRAIN_SMALL: the largest node the one-workgroup kernel takes; 0 sends every node through the multi-workgroup kernels.  Read once, at load.
const int g_small_limit = [] {
    const char* e = getenv("CORB_VOC_TRAIN_SMALL");
    if (!e || !*e) return VT_SMALL_DEFAULT;
    const long v = strtol(e, nullptr, 10);
    return (int)std::min<long>(std::max<long>(v, 0), VT_SMALL_MAX);
}();

// everything a call allocates, freed when it goes out of scope: the stream's work is waited for, the memory goes, then the stream
struct CallMem {
    OwnedStream stream; DevList dev;
    template <class T> hipError_t alloc(T** out, size_t n, bool zero = false)
    {
        hipError_t e = dev.add(out, n); if (e != hipSuccess) return e;
        return zero ? hipMemsetAsync(*out, 0, std::max(n, (size_t)1) * sizeof(T), stream) : hipSuccess;
    }
    template <class T> hipError_t upload(T** out, const std::vector<T>& src)
    {
        hipError_t e = alloc(out, src.size()); if (e != hipSuccess || src.empty()) return e;
        return hipMemcpyAsync(*out, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, stream);
    }
    void release(size_t keep) { dev.release(keep); }
    ~CallMem() { if (stream) (void)hipStreamSynchronize(stream); }
};

#define VTCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { corb_set_error("%s: %s failed: %s", who, #call, hipGetErrorString(e_)); return CORB_ERR_HIP; } } while (0)

int check_options(const char* who, const CorbVocTrainOptions* opt, long long n_features)
{
    if (!opt) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    const std::string err = vt_check_arguments(opt->k, opt->L, opt->max_iterations, n_features);
    if (!err.empty()) { corb_set_error("%s: %s", who, err.c_str()); return CORB_ERR_ARG; }
    return CORB_OK;
}

// d_desc: [N][4] on the device, already there on ow.stream; offset: host
int train(const char* who, CallMem& ow, const unsigned long long* d_desc, const int32_t* offset, int n_images, const CorbVocTrainOptions& opt, int device, CorbVoc** out, CorbVocTrainStats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int N = offset[n_images], k = opt.k, L = opt.L;
    VTCHK(vt_opt_in_lds());
    CorbVocTrainStats st; memset(&st, 0, sizeof st); st.small_limit = g_small_limit;
    int *d_perm, *d_perm_next, *d_min_d; unsigned char* d_assoc;
    VTCHK(ow.alloc(&d_perm, (size_t)N)); VTCHK(ow.alloc(&d_perm_next, (size_t)N)); VTCHK(ow.alloc(&d_min_d, (size_t)N)); VTCHK(ow.alloc(&d_assoc, (size_t)N));
    { std::vector<int> id(N); for (int i = 0; i < N; i++) id[i] = i; VTCHK(hipMemcpyAsync(d_perm, id.data(), (size_t)N * 4, hipMemcpyHostToDevice, ow.stream)); VTCHK(hipStreamSynchronize(ow.stream)); }
    const size_t keep = ow.dev.size();

    VtTree tree; const unsigned long long zero[VT_WORDS] = {0, 0, 0, 0}; tree.add(-1, zero);
    struct HostSeg { int node, begin, n; unsigned long long key; };
    std::vector<HostSeg> level{HostSeg{0, 0, N, 0}}, next;
    std::vector<VtSegDev> segs; std::vector<VtTileDev> tiles; std::vector<int> small_list, large_list;
    std::vector<unsigned long long> centres; std::vector<int> n_centres, iters, capped, empties, csize;
    unsigned long long pow21 = 1;
    for (int lv = 1; lv <= L && !level.empty(); lv++, pow21 *= 21) {
        const int S = (int)level.size();
        segs.resize(S); tiles.clear(); small_list.clear(); large_list.clear();
        int max_small = 1;
        for (int i = 0; i < S; i++) {
            const HostSeg& h = level[i];
            segs[i] = VtSegDev{h.begin, h.n, -1, 0, h.key};
            if (h.n <= g_small_limit) { small_list.push_back(i); max_small = std::max(max_small, h.n); continue; }
            segs[i].large = (int)large_list.size(); segs[i].tile_first = (int)tiles.size(); large_list.push_back(i);
            for (int b = 0; b < h.n; b += VT_TILE) tiles.push_back(VtTileDev{i, h.begin + b, std::min(VT_TILE, h.n - b)});
        }
        VtLevelDev d; memset(&d, 0, sizeof d);
        d.desc = d_desc; d.perm = d_perm; d.perm_next = d_perm_next; d.assoc = d_assoc; d.min_d = d_min_d;
        d.n_seg = S; d.n_small = (int)small_list.size(); d.n_large = (int)large_list.size(); d.n_tile = (int)tiles.size();
        d.k = k; d.max_iterations = opt.max_iterations; d.seed = opt.seed;
        VtSegDev* d_seg; int *d_small, *d_large; VtTileDev* d_tile;
        VTCHK(ow.upload(&d_seg, segs)); VTCHK(ow.upload(&d_small, small_list)); VTCHK(ow.upload(&d_large, large_list)); VTCHK(ow.upload(&d_tile, tiles));
        d.seg = d_seg; d.small_list = d_small; d.large_list = d_large; d.tile = d_tile;
        VTCHK(ow.alloc(&d.centres, (size_t)S * k * 4, true)); VTCHK(ow.alloc(&d.n_centres, (size_t)S, true)); VTCHK(ow.alloc(&d.iters, (size_t)S, true));
        VTCHK(ow.alloc(&d.capped, (size_t)S, true)); VTCHK(ow.alloc(&d.empties, (size_t)S, true)); VTCHK(ow.alloc(&d.csize, (size_t)S * k, true));
        VTCHK(ow.alloc(&d.tile_sum, (size_t)d.n_tile, true)); VTCHK(ow.alloc(&d.draw, (size_t)S, true)); VTCHK(ow.alloc(&d.seeding, (size_t)S, true));
        VTCHK(ow.alloc(&d.done, (size_t)S, true)); VTCHK(ow.alloc(&d.changed, (size_t)S, true)); VTCHK(ow.alloc(&d.counters, (size_t)d.n_large * k * 256, true));
        VTCHK(ow.alloc(&d.members, (size_t)d.n_large * k, true)); VTCHK(ow.alloc(&d.tile_hist, (size_t)d.n_tile * k, true)); VTCHK(ow.alloc(&d.running, 1, true));
        // every segment is partitioned in place: a child's range of the next permutation lies inside its parent's, and nothing outside a segment is ever read
        int launches = vt_launch_small(d, max_small, ow.stream);
        launches += vt_launch_seed(d, ow.stream);
        for (int it = 1; d.n_large > 0 && it <= opt.max_iterations; it++) {
            launches += vt_launch_iteration(d, it, ow.stream);
            int running = 0;
            VTCHK(hipMemcpyAsync(&running, d.running, 4, hipMemcpyDeviceToHost, ow.stream)); VTCHK(hipStreamSynchronize(ow.stream));
            if (!running) break;
            VTCHK(hipMemsetAsync(d.running, 0, 4, ow.stream));
        }
        launches += vt_launch_partition(d, ow.stream);
        VTCHK(hipGetLastError());
        centres.resize((size_t)S * k * 4); n_centres.resize(S); iters.resize(S); capped.resize(S); empties.resize(S); csize.resize((size_t)S * k);
        VTCHK(hipMemcpyAsync(centres.data(), d.centres, centres.size() * 8, hipMemcpyDeviceToHost, ow.stream)); VTCHK(hipMemcpyAsync(n_centres.data(), d.n_centres, (size_t)S * 4, hipMemcpyDeviceToHost, ow.stream));
        VTCHK(hipMemcpyAsync(iters.data(), d.iters, (size_t)S * 4, hipMemcpyDeviceToHost, ow.stream)); VTCHK(hipMemcpyAsync(capped.data(), d.capped, (size_t)S * 4, hipMemcpyDeviceToHost, ow.stream));
        VTCHK(hipMemcpyAsync(empties.data(), d.empties, (size_t)S * 4, hipMemcpyDeviceToHost, ow.stream)); VTCHK(hipMemcpyAsync(csize.data(), d.csize, csize.size() * 4, hipMemcpyDeviceToHost, ow.stream));
        VTCHK(hipStreamSynchronize(ow.stream));
        st.level_nodes[lv - 1] = S; st.level_launches[lv - 1] = launches; st.launches += launches; st.level_small_nodes[lv - 1] = d.n_small; st.level_large_nodes[lv - 1] = d.n_large;
        next.clear();
        for (int i = 0; i < S; i++) {
            const HostSeg& h = level[i]; const int nc = n_centres[i];
            if (nc < 1 || nc > k) { corb_set_error("%s: level %d: a node came back with %d centres", who, lv, nc); return CORB_ERR_OVERFLOW; }
            if (h.n <= k) st.trivial_nodes++;
            else {
                st.kmeans_nodes++; st.short_nodes += nc < k; st.capped_nodes += capped[i]; st.empty_cluster_events += empties[i];
                st.max_iterations_seen = std::max(st.max_iterations_seen, iters[i]); st.level_max_iterations[lv - 1] = std::max(st.level_max_iterations[lv - 1], iters[i]);
            }
            tree.child_first[h.node] = (int)tree.parent.size(); tree.child_count[h.node] = nc;
            int at = h.begin;
            for (int c = 0; c < nc; c++) {
                const int node = tree.add(h.node, &centres[((size_t)i * k + c) * 4]), m = csize[(size_t)i * k + c];
                if (lv < L && m > 1) next.push_back(HostSeg{node, at, m, vt_child_key(h.key, pow21, c)});
                at += m;
            }
            if (at != h.begin + h.n) { corb_set_error("%s: level %d: the clusters of a node hold %d of its %d features", who, lv, at - h.begin, h.n); return CORB_ERR_OVERFLOW; }
        }
        level.swap(next); std::swap(d_perm, d_perm_next);
        ow.release(keep);
    }

    // ---- the vocabulary, then setNodeWeights: the transform descent of every feature on the finished tree ----
    VtFlat flat; vt_renumber(tree, k, L, &flat);
    CorbVoc* v = new CorbVoc();
    const std::string err = bow_voc_build(k, L, 0, 0, (int)flat.parent.size(), flat.parent.data(), flat.is_leaf.data(), flat.descriptor.data(), flat.weight.data(), &v->host);
    if (!err.empty()) { corb_set_error("%s: the trained tree is not a vocabulary: %s", who, err.c_str()); delete v; return CORB_ERR_OVERFLOW; }
    CorbVoc* handle = nullptr;
    int rc = voc_finish(v, device, &handle, who); if (rc) return rc;
    auto fail = [&](int code) { corb_voc_destroy(handle); return code; };
#define VTCHK2(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { corb_set_error("%s: %s failed: %s", who, #call, hipGetErrorString(e_)); return fail(CORB_ERR_HIP); } } while (0)
    const int W = handle->host.n_words, words32 = (W + 31) / 32;
    int32_t *d_fword, *d_off; uint32_t* d_fnode; int* d_ni; BowSetDev* d_sets;
    VTCHK2(ow.alloc(&d_fword, (size_t)N)); VTCHK2(ow.alloc(&d_fnode, (size_t)N)); VTCHK2(ow.alloc(&d_ni, (size_t)W, true));
    { std::vector<int32_t> off(offset, offset + n_images + 1); VTCHK2(ow.upload(&d_off, off)); VTCHK2(hipStreamSynchronize(ow.stream)); }
    const int CH = 1 << 15;                                          // features per set of the descent: its sets are one grid dimension
    for (int first = 0; first < N; first += CH * BOW_MAX_SETS) {
        std::vector<BowSetDev> sets;
        for (int o = first; o < N && (int)sets.size() < BOW_MAX_SETS; o += CH) { BowSetDev t; memset(&t, 0, sizeof t); t.desc = d_desc + (size_t)o * 4; t.n = std::min(CH, N - o); t.feat_off = o; sets.push_back(t); }
        VTCHK2(ow.upload(&d_sets, sets)); VTCHK2(hipStreamSynchronize(ow.stream));
        corb_launch_bow_descend(handle->dev, d_sets, (int)sets.size(), std::min(CH, N - first), d_fword, d_fnode, ow.stream); st.launches++;
    }
    const size_t budget = (size_t)64 << 20;                          // bytes of bitmap per batch of images
    const int batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_images, budget / ((size_t)words32 * 4)));
    unsigned* d_bitmap; VTCHK2(ow.alloc(&d_bitmap, (size_t)batch * words32));
    for (int i0 = 0; i0 < n_images; i0 += batch) {
        const int cnt = std::min(batch, n_images - i0), f0 = offset[i0], fn = offset[i0 + cnt] - f0;
        if (fn <= 0) continue;
        VTCHK2(hipMemsetAsync(d_bitmap, 0, (size_t)cnt * words32 * 4, ow.stream));
        st.launches += vt_launch_count_images(d_fword, d_off, i0, cnt, f0, fn, words32, d_bitmap, d_ni, ow.stream);
    }
    VTCHK2(hipGetLastError());
    std::vector<int> ni(W);
    VTCHK2(hipMemcpyAsync(ni.data(), d_ni, (size_t)W * 4, hipMemcpyDeviceToHost, ow.stream)); VTCHK2(hipStreamSynchronize(ow.stream));
    vt_set_weights(handle->host, ni, n_images, &flat);                // log on the host
    VTCHK2(hipMemcpy((void*)handle->dev.word_weight, handle->host.word_weight.data(), (size_t)W * 8, hipMemcpyHostToDevice));
#undef VTCHK2
    st.nodes = handle->host.n_nodes; st.words = W;
    st.elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = st;
    *out = handle;
    return CORB_OK;
}

}  // namespace

extern "C" int corb_voc_train(const uint8_t* desc, const int32_t* offset, int n_images, const CorbVocTrainOptions* opt, int device, CorbVoc** out, CorbVocTrainStats* stats)
{
    const char* who = "corb_voc_train";
    if (!out || !offset || n_images < 1) { corb_set_error("%s: bad argument (at least one image, offset[n_images + 1])", who); return CORB_ERR_ARG; }
    *out = nullptr;
    if (offset[0] != 0) { corb_set_error("%s: offset[0] != 0", who); return CORB_ERR_ARG; }
    for (int i = 0; i < n_images; i++) if (offset[i + 1] < offset[i]) { corb_set_error("%s: offset decreases at image %d", who, i); return CORB_ERR_ARG; }
    int rc = check_options(who, opt, offset[n_images]); if (rc) return rc;
    if (!desc) { corb_set_error("%s: NULL array", who); return CORB_ERR_ARG; }
    rc = corb_select_device(device); if (rc) return rc;
    CallMem ow; unsigned long long* d_desc;
    VTCHK(ow.stream.create());
    const size_t N = (size_t)offset[n_images];
    VTCHK(ow.alloc(&d_desc, N * 4));
    VTCHK(hipMemcpyAsync(d_desc, desc, N * 32, hipMemcpyHostToDevice, ow.stream)); VTCHK(hipStreamSynchronize(ow.stream));
    return train(who, ow, d_desc, offset, n_images, *opt, device, out, stats);
}

extern "C" int corb_voc_train_store(CorbKfStore* s, const int32_t* slots, int n_slots, const CorbVocTrainOptions* opt, CorbVoc** out, CorbVocTrainStats* stats)
{
    const char* who = "corb_voc_train_store";
    if (!s || !out || n_slots < 1 || !slots) { corb_set_error("%s: bad argument (at least one slot)", who); return CORB_ERR_ARG; }
    *out = nullptr;
    for (int i = 0; i < n_slots; i++) {
        if (slots[i] < 0 || slots[i] >= s->capacity) { corb_set_error("%s: slot %d is outside the store", who, slots[i]); return CORB_ERR_ARG; }
        for (int j = 0; j < i; j++) if (slots[j] == slots[i]) { corb_set_error("%s: slot %d is listed twice", who, slots[i]); return CORB_ERR_ARG; }
    }
    if (!opt) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    int rc = corb_select_device(s->device); if (rc) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    std::vector<int32_t> offset(n_slots + 1, 0);
    for (int i = 0; i < n_slots; i++) {                                 // feature counts from the host mirror (read from the header once after a device-side fill)
        CorbKfStore::Host& h = s->host[slots[i]];
        if (!h.header_valid) {
            int hdr[4];
            VTCHK(hipMemcpyAsync(hdr, s->rec(slots[i]), sizeof(hdr), hipMemcpyDeviceToHost, s->stream)); VTCHK(hipStreamSynchronize(s->stream));
            if (hdr[0] < 0 || hdr[0] > s->F) { corb_set_error("%s: slot %d holds a corrupt record", who, slots[i]); return CORB_ERR_ARG; }
            h.n = hdr[0]; memcpy(&h.id, &hdr[2], 8);
        }
        offset[i + 1] = offset[i] + std::max(h.n, 0);
    }
    rc = check_options(who, opt, offset[n_slots]); if (rc) return rc;
    VTCHK(hipStreamSynchronize(s->stream));                             // pending fills of the records
    CallMem ow; unsigned long long* d_desc;
    VTCHK(ow.stream.create());
    VTCHK(ow.alloc(&d_desc, (size_t)offset[n_slots] * 4));
    for (int i = 0; i < n_slots; i++) {
        const size_t n = (size_t)(offset[i + 1] - offset[i]);
        if (n) VTCHK(hipMemcpyAsync(d_desc + (size_t)offset[i] * 4, s->rec(slots[i]) + s->L.desc, n * 32, hipMemcpyDeviceToDevice, ow.stream));
    }
    VTCHK(hipStreamSynchronize(ow.stream));
    return train(who, ow, d_desc, offset.data(), n_slots, *opt, s->device, out, stats);
}

extern "C" int corb_voc_get(const CorbVoc* v, int32_t* parent, int32_t* is_leaf, uint8_t* descriptor, double* weight, int cap_nodes, int* n_nodes)
{
    const char* who = "corb_voc_get";
    if (!v || !n_nodes || cap_nodes < 0) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    const int n = v->host.n_nodes - 1;
    *n_nodes = n;
    if (n > cap_nodes) { corb_set_error("%s: %d nodes, room for %d", who, n, cap_nodes); return CORB_ERR_OVERFLOW; }
    if (!parent || !is_leaf || !descriptor || !weight) { corb_set_error("%s: NULL array", who); return CORB_ERR_ARG; }
    VtFlat f; vt_flat_of(v->host, &f);
    memcpy(parent, f.parent.data(), (size_t)n * 4); memcpy(is_leaf, f.is_leaf.data(), (size_t)n * 4); memcpy(descriptor, f.descriptor.data(), (size_t)n * 32); memcpy(weight, f.weight.data(), (size_t)n * 8);
    return CORB_OK;
}

extern "C" int corb_voc_save_text(const CorbVoc* v, const char* path, int weight_digits)
{
    const char* who = "corb_voc_save_text";
    if (!v || !path || weight_digits < 0 || weight_digits > 17) { corb_set_error("%s: bad argument (weight_digits 0 .. 17)", who); return CORB_ERR_ARG; }
    VtFlat f; vt_flat_of(v->host, &f);
    const std::string text = vt_text(v->host.k, v->host.L, f, weight_digits);
    FILE* o = fopen(path, "wb");
    if (!o) { corb_set_error("%s: cannot open %s", who, path); return CORB_ERR_ARG; }
    const bool ok = fwrite(text.data(), 1, text.size(), o) == text.size();
    if (fclose(o) != 0 || !ok) { corb_set_error("%s: writing %s failed", who, path); return CORB_ERR_ARG; }
    return CORB_OK;
}
