// kfinsert_internal.h -- device-side argument blocks of keyframe insertion (kfinsert_kernels.hip, corb_kfinsert.cpp; include/corb_keyframe_insert.h)
#pragma once
#include "corb_internal.h"
#include "store_internal.h"
#include "device_util.h"

#define KFI_THREADS 1024

// corb_kfi_create_stereo_points: one workgroup.  out = [counts: 4 ints | order: cap ints | x3d: 3 cap floats | kind: cap bytes], read back as one block
struct KfiPointsDev {
    char* rec; int F;                                   // the record of (kf, slot)
    char* mirror; int mirror_F;                         // optional second record
    char* mp_base; size_t mp_bytes; int max_obs, mp_capacity; CorbIdTable idt;
    int cap, P;                                         // host-known feature count; the power of two >= max(cap, 1) the keys are padded to
    float th_depth; int mode, apply, first_mp_slot; unsigned long long first_mp_id; int client_id; long long frame_id;
    float fx, fy, cx, cy; int nlevels; float scale[CORB_MAX_LEVELS];
    int* counts;                                        // [0] visited, [1] created, [2] 1 = the map store is too small (nothing written)
    int* order; float* x3d; unsigned char* kind;
};
void corb_launch_kfi_points(const KfiPointsDev& d, hipStream_t s);

// corb_kfi_need_keyframe_counts.  kfid: id -> slot of the keyframes at hand (corb_launch_kf_index)
struct KfiCountsDev {
    const char* cur; int cur_F, n_cur; float th_depth;
    const char* ref; int ref_F, n_ref, min_obs;         // ref == nullptr: skipped
    const char* mp_base; size_t mp_bytes; int max_obs; CorbIdTable idt;
    const char* kf_base; size_t kf_bytes; int kf_F; CorbIdTable kfid;
    int* counts;                                        // [0] tracked close, [1] non-tracked close, [2] reference matches; zeroed before the launch
};
void corb_launch_kfi_counts(const KfiCountsDev& d, hipStream_t s);

// corb_kfi_process_new_keyframe: the kinds and the recent list in one workgroup, then (apply, room in every list) one wavefront per feature.
// out = [counts: 4 ints | recent: n ints | kind: n bytes]
struct KfiAssocDev {
    char* rec; int F, n;                                // the keyframe's record
    char* mp_base; size_t mp_bytes; int max_obs; CorbIdTable idt;
    char* kf_base; size_t kf_bytes; CorbIdTable kfid;   // the keyframes at hand (records of the same store as `rec`)
    CorbIdTable first;                                  // map-point slot -> lowest feature that holds it; prepared for corb_idtab_insert_min
    float scale_factor;
    int* counts;                                        // [0] added, [1] recent, [2] 1 = a kind-3 point's list is full (nothing written)
    int* recent; unsigned char* kind;
    int* mslot;                                         // [n] handle scratch: the map-point slot of a feature that holds a good point
    unsigned long long* desc;                           // [n][max_obs][4] handle scratch: the descriptors a point's observations contribute
};
void corb_launch_kfi_assoc(const KfiAssocDev& d, int apply, hipStream_t s);

// corb_kfi_map_point_culling: one workgroup.  out = [counts: 4 ints | kept: n ints | decision: n bytes]
struct KfiCullDev {
    const int* slots; int n; unsigned long long cur_kf_id; int th_obs, apply;
    char* mp_base; size_t mp_bytes; int max_obs;
    char* kf_base; size_t kf_bytes; int kf_F; CorbIdTable kfid;
    CorbIdTable first;                                  // slot -> first position in the list; prepared for corb_idtab_insert_min
    int* counts;                                        // [0] kept, [1] culled
    int* kept; unsigned char* decision;
};
void corb_launch_kfi_cull(const KfiCullDev& d, hipStream_t s);
