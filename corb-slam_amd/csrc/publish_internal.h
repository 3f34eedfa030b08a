// publish_internal.h -- what corb_publish.cpp hands to publish_kernels.hip (include/corb_map_publish.h): the device view of one pack and of one apply
#pragma once
#include "store_internal.h"
#include "device_util.h"
#include "../../include/corb_map_publish.h"

#define PUB_WG 256                      // one entry per lane; the ordered compaction counts, scans and scatters per workgroup of this size

// the head of an apply's output block (read back with it): the verdicts the kernels hand to one another through device memory, then the client's transform
struct PubState {
    int found;                          // the client's id is in section E
    int n_ins[2];                       // accepted entries of A, of B
    int n_upd[2];                       // kind-2 entries of C, of D
    int overflow;                       // bit 0: more accepted keyframes than room, bit 1: map points
    int go;                             // the write phases run: found, apply, no overflow
    int dup;                            // the rebuilt id index met one id twice
    float T[16], Tinv[16];
};
static_assert(sizeof(PubState) == 160, "PubState heads the output block: 16-byte multiple");

struct PubPackDev {
    const char* kf_base; size_t kf_bytes; const char* mp_base; size_t mp_bytes;
    const int* upd_kf; int n_upd_kf; const int* upd_mp; int n_upd_mp;
    char* sec_c; char* sec_d;
};

// side 0 = keyframes (sections A, C), side 1 = map points (B, D)
struct PubSide {
    const char* sec_new; int n_new; size_t rec_bytes;          // section A / B
    const char* sec_upd; int n_upd;                            // section C / D
    char* base; int capacity, free_first, room;                // the destination store
    CorbIdTable held;                                          // id -> slot of what the store holds (keyframes: built by the call; map points: the map's index)
    CorbIdTable first, last;                                   // id -> lowest position among the would-be accepted of A / B; id -> n - 1 - highest position of the kind-2 of C / D
    unsigned char* kind_new; unsigned char* kind_upd;          // output block
    int* new_slots;                                            // output block: [min(n_new, room)]
    int* rank; int* src;                                       // [n_new] rank of an accepted entry among the accepted (-1: none); message position of the k-th accepted
    int* target;                                               // [n_upd] the slot a kind-2 entry writes
    int* wg_cnt; int* wg_off; int* scan_scratch;               // [n_wg], [n_wg + 1], corb_scan_scratch_ints(n_wg)
};
struct PubApplyDev {
    PubState* st;
    const CorbPublishTransform* sec_e; int n_trans; int client_id; int apply;
    PubSide s[2];
    int* kf_hdr;                                               // output block: {n, n_nodes, id lo, id hi} of the k-th accepted keyframe, [min(n_new, room)][4]
    int mp_first, mp_n; CorbIdTable new_index;                 // the map's id index after the call: rebuilt into this table over [mp_first, mp_first + mp_n + accepted)
};

void pub_launch_pack_poses(const PubPackDev& d, hipStream_t s);
// everything of an apply behind the keyframe id table and the cleared tables: classify, compact, gate, update decisions, then the gated writes
void pub_launch_apply(const PubApplyDev& d, hipStream_t s);
