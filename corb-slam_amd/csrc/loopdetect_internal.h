// loopdetect_internal.h -- LoopClosing::DetectLoop on records (corb_loopdetect.cpp, loopdetect_kernels.hip): the detector's device state as the kernels see it, launchers
#pragma once
#include "corb_internal.h"
#include "store_internal.h"
#include "covis_internal.h"
#include "bow_internal.h"
#include "corb_loop_detect.h"

#define LD_T 256                             // threads of every workgroup here
#define LD_MODE_FULL 0                       // what ld_begin_kernel decides for the keyframe at hand
#define LD_MODE_GAP  1
#define LD_MODE_ERR  2

// what LoopClosing holds between calls, and the keyframe at hand
struct LdState {
    unsigned long long last_loop;            // mLastLoopKFid
    int th;                                  // mnCovisibilityConsistencyTh
    int cur;                                 // which of the two group buffers is mvConsistentGroups
    int n_groups;
    int mode;                                // LD_MODE_* of the keyframe at hand
};
// the front of the read-back block: the queue's running state
struct LdHead { int stop, consumed, pad[2]; };
// one keyframe's slice of the read-back block: LdItem, then cand_entries / cand_slots / enough of max_cand ints each
struct LdItem { CorbLoopDetectResult r; int status; int pad[2]; };
static_assert(sizeof(LdItem) == 32, "LdItem is 32 bytes");

struct LdDev {
    const char* kf_base; size_t kf_bytes; int n_slots, W;                // the graph's keyframe store; words of a group's bit set
    CorbIdTable kfid;                                                    // mnId -> slot, rebuilt by every detect call
    CovisRows R;                                                         // the graph's rows
    int* slot_entry; int* entry_slot; int n_entries;                     // [n_slots], [n_entries]: the binding, -1 = none
    LdState* st;
    unsigned long long* grp_bits; int* grp_cnt;                          // [2][max_groups][W], [2][max_groups]
    unsigned long long* cand_bits;                                       // [max_cand][W]
    unsigned char* cons;                                                 // [max_cand][max_groups] Consistent(i, iG)
    int* first;                                                          // [max_groups] the first candidate consistent with previous group iG, or INT_MAX
    int* src;                                                            // [max_groups] the candidate whose group new group j is
    int* pos; int* any; int* en; int* epos;                              // [max_cand + 1] per candidate: new groups (then offsets), consistent with some group, enough (then offsets)
    int* score_list;                                                     // [M] the entries minScore is taken over
    BowLoopQuery* q;
    char* block; size_t item_bytes;                                      // LdHead (256 bytes) | items
    int max_cand, max_groups;

    __host__ __device__ LdHead* head() const { return reinterpret_cast<LdHead*>(block); }
    __host__ __device__ LdItem* item(int k) const { return reinterpret_cast<LdItem*>(block + 256 + (size_t)k * item_bytes); }
    __host__ __device__ int* item_ints(int k, int which) const { return reinterpret_cast<int*>(block + 256 + (size_t)k * item_bytes + sizeof(LdItem)) + (size_t)which * max_cand; }
};

// the kernels of keyframe k of a call, in stream order: begin | the database's loop query (corb_launch_kfdb_loop_query) | groups | close
void ld_launch_begin(const LdDev& d, const BowDbDev& db, int k, int slot, hipStream_t s);
void ld_launch_groups(const LdDev& d, const BowDbDev& db, int k, hipStream_t s);
void ld_launch_close(const LdDev& d, const BowDbDev& db, int k, int entry, unsigned int seq, hipStream_t s);
void ld_launch_drop_slot(const LdDev& d, int slot, hipStream_t s);
