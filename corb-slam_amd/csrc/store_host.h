// store_host.h -- host-side objects of the device-resident stores (corb_store.cpp, corb_comm.cpp, corb_ba_store.cpp)
#pragma once
#include "store_internal.h"
#include <mutex>
#include <vector>
#include "owned_hip.h"

struct CorbKfStore {
    int device = 0, capacity = 0, F = 0;
    RecLayout L{1};
    OwnedStream stream;
    OwnedEvent ev;
    DevMem mem;                               // [capacity][L.bytes]
    std::mutex mu;
    struct Host { int n = -1, n_nodes = 0; unsigned long long id = 0; std::vector<uint32_t> node_id; bool header_valid = false; };
    std::vector<Host> host;                   // host mirror of the small parts (counts, vocabulary node ids)
    char* base() const { return mem.as<char>(); }
    char* rec(int slot) const { return base() + (size_t)slot * L.bytes; }
};

struct CorbMpStore {
    int device = 0, capacity = 0, O = 0;      // O = max observations per map point
    MpLayout L{1};
    OwnedStream stream;
    DevMem mem;                               // [capacity][L.bytes]
    std::mutex mu;
    OwnedIdTable idt;                         // mnId -> slot of the slots indexed by corb_mp_store_build_index (tracking calls on records); keys == nullptr: none
    int idt_first = 0, idt_n = 0; bool idt_valid = false;      // cleared by whatever rewrites record headers (put, incoming push)
    // scratch of corb_local_ba_store (a call per keyframe: no hipMalloc / hipFree per call): device arena + page-locked staging, grown between calls to
    // what the largest call asked for (up to 256 MB / 64 MB; beyond that the call allocates)
    DevMem lba_dev; size_t lba_dev_want = 0;
    PinnedMem lba_host; size_t lba_host_want = 0;
    OwnedEvent lba_event;                          // the window's graph is complete (corb_local_ba_store: this store's stream -> the optimiser's)
    char* base() const { return mem.as<char>(); }
    char* rec(int slot) const { return base() + (size_t)slot * L.bytes; }
};

// slot in range and host[slot] current (counts and node ids read from the record once after a device-side fill); under s->mu (corb_store.cpp)
int kf_store_slot_ready(CorbKfStore* s, int slot, const char* who);

// the vocabulary nodes two FeatureVectors share (both ascend in the node id): positions in a and in b -- what the BoW-guided matchers on slots walk
inline void common_nodes(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, std::vector<int>& pa, std::vector<int>& pb)
{
    size_t i = 0, j = 0;
    while (i < a.size() && j < b.size()) { if (a[i] == b[j]) { pa.push_back((int)i++); pb.push_back((int)j++); } else if (a[i] < b[j]) i++; else j++; }
}
