// corb_trajectory.cpp -- C-ABI host side of include/corb_trajectory.h: the per-frame log of Tracking::Track, KeyFrame::mTcp / mTimeStamp per slot, and the three
// trajectory dumps of System.cc on the device.  The object owns its device memory, its page-locked staging and its stream: no call here opens a workspace lane.
// Locks: the graph, then the keyframe stores by address (record_locks.h).  The log's length is the host's: an append passes the index it writes.
// Order on the device: an append runs on the frame store's stream (or the object's) behind the event of the append before it; every other call runs on the
// object's stream behind that event and returns synchronised.
#include "traj_internal.h"
#include "covis_host.h"
#include "record_call.h"
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct CorbTrajectory {
    CorbCovis* g = nullptr;
    int device = 0, capacity = 0, n_slots = 0, n = 0;      // n: entries in the log
    size_t N = 0;                                         // rows the export block has room for: max(capacity, n_slots)
    OwnedStream stream;
    OwnedEvent ev; bool ev_set = false;                   // the last append
    DevMem mem;                                           // everything TrajDev points into
    PinnedMem back;                                       // the export block's host side
    TrajDev d{};
    size_t o_rows = 0, o_times = 0, o_index = 0, block_bytes = 0;
};

namespace {
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// one call's opening: the device, the locks (the graph, the graph's store, a frame store), the streams this call's kernels read behind
struct TrajCall : RecordCall {
    int open(const char* who, CorbTrajectory* t, bool args_ok, CorbKfStore* frames = nullptr)
    {
        if (!t || !args_ok) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
        if (frames && frames->device != t->device) { corb_set_error("%s: the frame store lives on another device", who); return CORB_ERR_ARG; }
        int rc = corb_select_device(t->device); if (rc) return rc;
        hold(&t->g->mu, t->g->kf, frames, nullptr);
        t->d.kf_base = t->g->kf->base(); t->d.parent = t->g->T.parent;
        return CORB_OK;
    }
    // the object's stream behind the graph's store and the last append
    int behind(CorbTrajectory* t)
    {
        HIPCHK(hipStreamSynchronize(t->g->kf->stream));
        if (t->ev_set) HIPCHK(hipStreamWaitEvent(t->stream, t->ev, 0));
        return CORB_OK;
    }
};
int slot_held(const char* who, const CorbKfStore* kf, int slot)
{
    if (slot < 0 || slot >= kf->capacity) { corb_set_error("%s: slot %d of %d", who, slot, kf->capacity); return CORB_ERR_ARG; }
    if (record_slot_count(who, kf, slot) < 0) return CORB_ERR_ARG;
    if (kf->host[slot].n == 0) { corb_set_error("%s: slot %d holds no feature: it is not a keyframe", who, slot); return CORB_ERR_ARG; }
    return CORB_OK;
}
int table_copy(const char* who, CorbTrajectory* t, int slot, void* host, void* dev, size_t bytes, bool to_device)
{
    TrajCall c; int rc = c.open(who, t, host != nullptr); if (rc) return rc;
    if (slot < 0 || slot >= t->n_slots) { corb_set_error("%s: slot %d of %d", who, slot, t->n_slots); return CORB_ERR_ARG; }
    rc = c.behind(t); if (rc) return rc;
    if (to_device) HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, t->stream));
    else HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return CORB_OK;
}

// %.pf of the value widened to double is what `f << fixed << setprecision(p) << float` writes
void put_value(std::string& s, double v, int precision)
{
    char b[400];
    const int k = snprintf(b, sizeof(b), "%.*f", precision, v);
    s.append(b, (size_t)std::max(k, 0));
}
int format_text(int kind, const float* rows, const double* times, int n, std::string& s)
{
    if (kind < 0 || kind > 2 || n < 0 || (n > 0 && (!rows || (kind != 0 && !times)))) { corb_set_error("corb_traj_format_rows: kind %d (0 .. 2), %d rows, NULL arrays", kind, n); return CORB_ERR_ARG; }
    const int w = kind == 0 ? 12 : 7, p = kind == 2 ? 7 : 9;
    s.clear(); s.reserve((size_t)n * (size_t)(w + 1) * 16);
    for (int r = 0; r < n; r++) {
        if (kind != 0) { put_value(s, times[r], 6); s.push_back(' '); }
        for (int j = 0; j < w; j++) { put_value(s, (double)rows[(size_t)r * w + j], p); s.push_back(j + 1 < w ? ' ' : '\n'); }
    }
    return CORB_OK;
}
}  // namespace

extern "C" int corb_traj_create(CorbCovis* g, int capacity_frames, CorbTrajectory** out)
{
    if (!out || !g || capacity_frames < 1) { corb_set_error("corb_traj_create: bad argument (capacity_frames >= 1)"); return CORB_ERR_ARG; }
    *out = nullptr;
    int rc = corb_select_device(g->device); if (rc) return rc;
    CorbTrajectory* t = new CorbTrajectory();
    t->g = g; t->device = g->device; t->capacity = capacity_frames; t->n_slots = g->kf->capacity; t->N = (size_t)std::max(t->capacity, t->n_slots);
    const size_t S = (size_t)t->n_slots, Cn = (size_t)t->capacity, N = t->N;
    t->o_rows = al256(sizeof(TrajHead)); t->o_times = t->o_rows + al256(N * 12 * 4); t->o_index = t->o_times + al256(N * 8); t->block_bytes = t->o_index + al256(N * 8);
    size_t o = 0;
    const size_t o_block = o; o += t->block_bytes;
    const size_t o_entries = o; o += al256(Cn * sizeof(CorbTrajEntry));
    const size_t o_tcp = o; o += al256(S * 64);
    const size_t o_time = o; o += al256(S * 8);
    const size_t o_id = o; o += al256(S * 8);
    const size_t o_tcw = o; o += al256(S * 64);
    const size_t o_trw = o; o += al256(S * 64);
    const size_t o_flags = o; o += al256(S * 4);
    const size_t o_held = o; o += al256(S * 4);
    const size_t o_pslot = o; o += al256(S * 4);
    const size_t o_chain = o; o += al256(S * 4);
    const size_t o_valid = o; o += al256((Cn + 1) * 4);
    const size_t o_pos = o; o += al256((Cn + 1) * 4);
    const size_t o_scan = o; o += al256(corb_scan_scratch_ints(Cn) * 4);
    const size_t o_status = o; o += 256;
    if (t->stream.create() != hipSuccess || t->ev.create(hipEventDisableTiming) != hipSuccess || t->mem.room(o) != hipSuccess || t->back.room(t->block_bytes) != hipSuccess) {
        corb_set_error("corb_traj_create: %d frames over %d slots: allocation failed", capacity_frames, t->n_slots); delete t; return CORB_ERR_HIP;
    }
    char* m = t->mem.as<char>();
    TrajDev& d = t->d;
    d.kf_base = g->kf->base(); d.kf_bytes = g->kf->L.bytes; d.n_slots = t->n_slots; d.parent = g->T.parent;
    d.entries = reinterpret_cast<CorbTrajEntry*>(m + o_entries); d.capacity = t->capacity;
    d.Tcp = reinterpret_cast<float*>(m + o_tcp); d.time = reinterpret_cast<double*>(m + o_time);
    d.flags = reinterpret_cast<unsigned int*>(m + o_flags); d.held = reinterpret_cast<int*>(m + o_held); d.id = reinterpret_cast<unsigned long long*>(m + o_id);
    d.parent_slot = reinterpret_cast<int*>(m + o_pslot); d.Tcw = reinterpret_cast<float*>(m + o_tcw); d.Trw = reinterpret_cast<float*>(m + o_trw); d.chain = reinterpret_cast<int*>(m + o_chain);
    d.valid = reinterpret_cast<int*>(m + o_valid); d.pos = reinterpret_cast<int*>(m + o_pos); d.scan_scratch = reinterpret_cast<int*>(m + o_scan);
    d.head = reinterpret_cast<TrajHead*>(m + o_block); d.rows = reinterpret_cast<float*>(m + o_block + t->o_rows); d.times = reinterpret_cast<double*>(m + o_block + t->o_times);
    d.index = reinterpret_cast<int*>(m + o_block + t->o_index);
    d.status = reinterpret_cast<int*>(m + o_status);
    // mTcp is left uninitialised by the reference (KeyFrame.cc:63); here it starts as the identity, as mTcwBefGBA does in the graph
    std::vector<float> eye(S * 16, 0.f);
    for (size_t i = 0; i < S; i++) eye[i * 16] = eye[i * 16 + 5] = eye[i * 16 + 10] = eye[i * 16 + 15] = 1.f;
    if (hipMemsetAsync(m, 0, o, t->stream) != hipSuccess || hipMemcpyAsync(d.Tcp, eye.data(), eye.size() * 4, hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipStreamSynchronize(t->stream) != hipSuccess) { corb_set_error("corb_traj_create: the tables' initialisation failed"); delete t; return CORB_ERR_HIP; }
    *out = t;
    return CORB_OK;
}
extern "C" void corb_traj_destroy(CorbTrajectory* t)
{
    if (t && t->ev_set) { (void)corb_select_device(t->device); (void)hipEventSynchronize(t->ev); }      // an append may still run on a frame store's stream
    handle_destroy(t);
}

extern "C" int corb_traj_reset(CorbTrajectory* t)
{
    TrajCall c; int rc = c.open("corb_traj_reset", t, true); if (rc) return rc;
    t->n = 0;                                                                            // mlRelativeFramePoses.clear(); mlpReferences.clear(); mlFrameTimes.clear(); mlbLost.clear();
    return CORB_OK;
}

extern "C" int corb_traj_append(CorbTrajectory* t, CorbKfStore* frames, int cur_slot, int ref_slot, const float* Tcr, double timestamp, int lost)
{
    const char* who = "corb_traj_append";
    const bool copy = cur_slot == -1, compute = !copy && !Tcr;
    TrajCall c; int rc = c.open(who, t, cur_slot >= -1 && (!compute || frames), copy ? nullptr : frames); if (rc) return rc;
    CorbKfStore* kf = t->g->kf;
    if (copy && t->n == 0) { corb_set_error("%s: cur_slot = -1 on an empty log: there is no last entry to repeat", who); return CORB_ERR_ARG; }
    if (!copy) {
        rc = slot_held(who, kf, ref_slot); if (rc) return rc;
        if (compute && cur_slot >= frames->capacity) { corb_set_error("%s: frame slot %d of %d", who, cur_slot, frames->capacity); return CORB_ERR_ARG; }
        if (compute && record_slot_count(who, frames, cur_slot) < 0) return CORB_ERR_ARG;
    }
    if (t->n >= t->capacity) { corb_set_error("%s: the log holds %d entries, its capacity", who, t->n); return CORB_ERR_CAPACITY; }
    hipStream_t s = (!copy && frames) ? (hipStream_t)frames->stream : (hipStream_t)t->stream;
    if (!copy && (hipStream_t)kf->stream != s) HIPCHK(hipStreamSynchronize(kf->stream));              // the reference's record may still be filling
    if (t->ev_set) HIPCHK(hipStreamWaitEvent(s, t->ev, 0));
    traj_launch_append(t->d, copy ? 2 : (compute ? 1 : 0), t->n, compute ? frames->rec(cur_slot) : nullptr, copy ? 0 : ref_slot, Tcr, timestamp, lost, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(t->ev, s)); t->ev_set = true;
    t->n++;
    return CORB_OK;
}

extern "C" int corb_traj_set_keyframe_time(CorbTrajectory* t, int slot, double timestamp)
{
    return table_copy("corb_traj_set_keyframe_time", t, slot, &timestamp, t ? t->d.time + slot : nullptr, 8, true);
}
extern "C" int corb_traj_get_keyframe_time(CorbTrajectory* t, int slot, double* timestamp)
{
    return table_copy("corb_traj_get_keyframe_time", t, slot, timestamp, t ? t->d.time + slot : nullptr, 8, false);
}
extern "C" int corb_traj_set_tcp(CorbTrajectory* t, int slot, const float* Tcp)
{
    return table_copy("corb_traj_set_tcp", t, slot, const_cast<float*>(Tcp), t ? t->d.Tcp + (size_t)slot * 16 : nullptr, 64, true);
}
extern "C" int corb_traj_get_tcp(CorbTrajectory* t, int slot, float* Tcp)
{
    return table_copy("corb_traj_get_tcp", t, slot, Tcp, t ? t->d.Tcp + (size_t)slot * 16 : nullptr, 64, false);
}

extern "C" int corb_traj_set_bad_pose(CorbTrajectory* t, int slot)
{
    const char* who = "corb_traj_set_bad_pose";
    TrajCall c; int rc = c.open(who, t, true); if (rc) return rc;
    rc = slot_held(who, t->g->kf, slot); if (rc) return rc;
    rc = c.behind(t); if (rc) return rc;
    traj_launch_set_bad_pose(t->d, slot, t->stream);
    HIPCHK(hipGetLastError());
    int* st = t->back.as<int>();
    HIPCHK(hipMemcpyAsync(st, t->d.status, 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    if (*st) { corb_set_error("%s: the keyframe in slot %d has no parent, or one the store does not hold; Tcp is unchanged", who, slot); return CORB_ERR_ARG; }
    return CORB_OK;
}

extern "C" int corb_traj_get_entries(CorbTrajectory* t, CorbTrajEntry* entries, int cap, int* n)
{
    const char* who = "corb_traj_get_entries";
    TrajCall c; int rc = c.open(who, t, n && cap >= 0); if (rc) return rc;
    *n = t->n;
    if (t->n > cap) { corb_set_error("%s: the log holds %d entries, cap = %d", who, t->n, cap); return CORB_ERR_CAPACITY; }
    if (t->n == 0) return CORB_OK;
    if (!entries) { corb_set_error("%s: NULL entries", who); return CORB_ERR_ARG; }
    rc = c.behind(t); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(entries, t->d.entries, (size_t)t->n * sizeof(CorbTrajEntry), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return CORB_OK;
}

namespace {
// the frames' export into the object's staging; the caller holds the locks.  *n and *stats are set whenever CORB_OK or CORB_ERR_CAPACITY comes back
int frames_export(const char* who, CorbTrajectory* t, TrajCall& c, int origin_slot, int format, int cap, int* n, CorbTrajStats* stats)
{
    if (origin_slot >= 0) { int rc = slot_held(who, t->g->kf, origin_slot); if (rc) return rc; }
    int rc = c.behind(t); if (rc) return rc;
    const int ne = t->n, w = format == 0 ? 12 : 7;
    traj_launch_frames(t->d, ne, origin_slot, format, t->stream);
    HIPCHK(hipGetLastError());
    char* dev = reinterpret_cast<char*>(t->d.head); char* host = t->back.as<char>();
    HIPCHK(hipMemcpyAsync(host, dev, sizeof(TrajHead), hipMemcpyDeviceToHost, t->stream));
    if (ne > 0) {
        HIPCHK(hipMemcpyAsync(host + t->o_rows, dev + t->o_rows, (size_t)ne * w * 4, hipMemcpyDeviceToHost, t->stream));
        HIPCHK(hipMemcpyAsync(host + t->o_times, dev + t->o_times, (size_t)ne * 8, hipMemcpyDeviceToHost, t->stream));
        HIPCHK(hipMemcpyAsync(host + t->o_index, dev + t->o_index, (size_t)ne * 4, hipMemcpyDeviceToHost, t->stream));
    }
    HIPCHK(hipStreamSynchronize(t->stream));
    const TrajHead& H = *reinterpret_cast<const TrajHead*>(host);
    if (ne > 0 && H.status) { corb_set_error("%s: no held keyframe without CORB_KF_BAD can be the origin", who); return CORB_ERR_ARG; }
    *n = ne > 0 ? H.n_rows : 0;
    if (stats) { if (ne > 0) *stats = H.stats; else memset(stats, 0, sizeof(*stats)); }
    if (*n > cap) { corb_set_error("%s: %d rows, cap = %d", who, *n, cap); return CORB_ERR_CAPACITY; }
    return CORB_OK;
}
int keyframes_export(const char* who, CorbTrajectory* t, TrajCall& c, int cap, int* n)
{
    int rc = c.behind(t); if (rc) return rc;
    traj_launch_keyframes(t->d, t->stream);
    HIPCHK(hipGetLastError());
    char* dev = reinterpret_cast<char*>(t->d.head); char* host = t->back.as<char>();
    const size_t S = (size_t)t->n_slots;
    HIPCHK(hipMemcpyAsync(host, dev, sizeof(TrajHead), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(host + t->o_rows, dev + t->o_rows, S * 7 * 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(host + t->o_times, dev + t->o_times, S * 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(host + t->o_index, dev + t->o_index, S * 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    *n = std::min(std::max(reinterpret_cast<const TrajHead*>(host)->n_rows, 0), t->n_slots);
    if (*n > cap) { corb_set_error("%s: %d keyframes, cap = %d", who, *n, cap); return CORB_ERR_CAPACITY; }
    return CORB_OK;
}
}  // namespace

extern "C" int corb_traj_frames(CorbTrajectory* t, int origin_slot, int format, float* rows, double* times, int32_t* entry_index, int cap, int* n, CorbTrajStats* stats)
{
    const char* who = "corb_traj_frames";
    TrajCall c; int rc = c.open(who, t, n && cap >= 0 && (format == 0 || format == 1) && origin_slot >= -1 && (rows || cap == 0)); if (rc) return rc;
    rc = frames_export(who, t, c, origin_slot, format, cap, n, stats); if (rc) return rc;
    const char* host = t->back.as<char>(); const size_t k = (size_t)*n;
    if (k) memcpy(rows, host + t->o_rows, k * (format == 0 ? 12 : 7) * 4);
    if (k && times) memcpy(times, host + t->o_times, k * 8);
    if (k && entry_index) memcpy(entry_index, host + t->o_index, k * 4);
    return CORB_OK;
}

extern "C" int corb_traj_keyframes(CorbTrajectory* t, float* rows, double* times, uint64_t* ids, int cap, int* n)
{
    const char* who = "corb_traj_keyframes";
    TrajCall c; int rc = c.open(who, t, n && cap >= 0 && (rows || cap == 0)); if (rc) return rc;
    rc = keyframes_export(who, t, c, cap, n); if (rc) return rc;
    const char* host = t->back.as<char>(); const size_t k = (size_t)*n;
    if (k) memcpy(rows, host + t->o_rows, k * 7 * 4);
    if (k && times) memcpy(times, host + t->o_times, k * 8);
    if (k && ids) memcpy(ids, host + t->o_index, k * 8);
    return CORB_OK;
}

extern "C" int corb_traj_format_rows(int kind, const float* rows, const double* times, int n, char* buf, size_t cap, size_t* len)
{
    if (!len) { corb_set_error("corb_traj_format_rows: NULL len"); return CORB_ERR_ARG; }
    std::string s;
    int rc = format_text(kind, rows, times, n, s); if (rc) return rc;
    *len = s.size();
    if (!buf || s.size() > cap) { corb_set_error("corb_traj_format_rows: the text is %zu bytes, cap = %zu", s.size(), buf ? cap : (size_t)0); return CORB_ERR_CAPACITY; }
    memcpy(buf, s.data(), s.size());
    return CORB_OK;
}

extern "C" int corb_traj_save(CorbTrajectory* t, int origin_slot, int kind, const char* path)
{
    const char* who = "corb_traj_save";
    std::string text;
    {
        TrajCall c; int rc = c.open(who, t, path && kind >= 0 && kind <= 2 && origin_slot >= -1); if (rc) return rc;
        int n = 0;
        if (kind == 2) rc = keyframes_export(who, t, c, t->n_slots, &n);
        else rc = frames_export(who, t, c, origin_slot, kind, t->capacity, &n, nullptr);
        if (rc) return rc;
        const char* host = t->back.as<char>();
        rc = format_text(kind, reinterpret_cast<const float*>(host + t->o_rows), reinterpret_cast<const double*>(host + t->o_times), n, text); if (rc) return rc;
    }
    FILE* f = fopen(path, "wb");
    if (!f) { corb_set_error("%s: cannot open %s: %s", who, path, strerror(errno)); return CORB_ERR_ARG; }
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) { corb_set_error("%s: writing %s failed", who, path); return CORB_ERR_ARG; }
    return CORB_OK;
}
