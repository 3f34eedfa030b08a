// comm_internal.h -- the communicator object (include/corb_accel.h: corb_comm_*) as the translation units that move records between ranks see it: the map push
// (corb_comm.cpp, which defines the two transports' methods) and the map publish (corb_publish.cpp).  Host code only.
#pragma once
#include "store_host.h"
#include "corb_workspace.h"
#include "owned_hip.h"
#include <algorithm>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

typedef struct ncclComm* ncclComm_t;
struct Msg { void* ptr; size_t bytes; int peer; };

// in-process transport: `world` communicators share one hub; every rank is driven by its own host thread
struct LocalHub {
    int world = 1;
    std::mutex mu; std::condition_variable cv;
    int arrived = 0; unsigned long long generation = 0;
    std::vector<int> table;                              // all-gather staging
    std::vector<std::vector<Msg>> posted;                // posted[sender] = the sends of the current exchange (peer = receiver)
    const void* publish_src[2] = {nullptr, nullptr};     // the stores the root of the running map publish reads (corb_publish.cpp: a receiver may not write them)
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const unsigned long long g = generation;
        if (++arrived == world) { arrived = 0; generation++; cv.notify_all(); }
        else cv.wait(lk, [&] { return generation != g; });
    }
};

struct CorbComm {
    int rank = 0, world = 1, device = 0;
    OwnedStream stream;
    // RCCL
    ncclComm_t comm = nullptr; DevMem d_ints; int d_ints_cap = 0;
    // in-process
    std::shared_ptr<LocalHub> hub;
    // staging buffers of the outgoing records (kept between pushes: a hipMalloc / hipFree pair per push cost more than the 1.5 MB transfer it served)
    DevMem stage_kf, stage_mp, stage_slots;
    // asynchronous push: the root's layout (corb_map_push_setup) and the push in flight
    bool layout_set = false; int layout_root = -1, layout_kf_cap = 0, layout_mp_cap = 0, layout_kf_bytes = 0, layout_mp_bytes = 0;
    std::vector<int32_t> layout_kf_first, layout_mp_first;
    const CorbKfStore* layout_kf_store = nullptr; const CorbMpStore* layout_mp_store = nullptr;      // the root's stores the layout describes (begin must be handed the same)
    OwnedEvent push_done; bool in_flight = false; int flight_rc = CORB_OK;
    CorbMapPush flight_push; int flight_root = -1; std::vector<CorbPushHeader> flight_hdr;
    // a staging buffer holds at least `need` bytes: exactly that when it grows, 1 MB at the least
    int room(DevMem& buf, size_t need) {
        const size_t grow = std::max(need, (size_t)1 << 20);
        if (buf.room(need, grow) != hipSuccess) { corb_set_error("corb_comm: staging buffer of %zu bytes could not be allocated", grow); return CORB_ERR_HIP; }
        return CORB_OK;
    }

    // every rank contributes n ints; all[r * n + k] = rank r's k-th
    int all_gather(const int* mine, int n, int* all);
    // device buffers; messages between a pair of ranks match in posting order; returns when this rank's sends and receives are complete
    // wait = false (RCCL only): the messages are enqueued on the communicator's stream, completion is the caller's event
    // dst_a / dst_b (in-process transport): the mutexes of the stores this rank RECEIVES into, held while it copies -- between the two barriers, where no other
    // rank holds a store lock (each took its source stores' only while it packed, before the first barrier): ranks that share stores cannot deadlock
    int exchange(const std::vector<Msg>& sends, const std::vector<Msg>& recvs, bool wait = true, std::mutex* dst_a = nullptr, std::mutex* dst_b = nullptr);
};
