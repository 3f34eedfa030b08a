// voctrain_internal.h -- device views and launchers shared by voctrain_kernels.hip and corb_voctrain.cpp (vocabulary training, include/corb_voc_train.h)
#pragma once
#include "bow_internal.h"
#include "voctrain_math.h"

#define VT_TILE 1024                // positions per workgroup of the multi-workgroup kernels: 256 lanes x 4
#define VT_SMALL_MAX 3072           // the largest node the one-workgroup kernel can hold: 37 bytes of LDS per descriptor + 24 KiB of counters and centres, of 160 KiB
#define VT_SMALL_DEFAULT 2048       // CORB_VOC_TRAIN_SMALL when unset: 100 KiB of LDS at k = 20

// one active node of a level on the device: its descriptors are perm[begin .. begin + n) in original relative order.  large >= 0: its ordinal among the nodes the
// multi-workgroup kernels take, and the first of its ceil(n / VT_TILE) tiles; large < 0: the one-workgroup kernel takes it.
struct VtSegDev { int begin, n, large, tile_first; unsigned long long key; };
struct VtTileDev { int seg, begin, n; };

struct VtLevelDev {
    const unsigned long long* desc;     // [N][4] every training feature
    const int* perm; int* perm_next;    // [N]
    const VtSegDev* seg; int n_seg;
    const int* small_list; int n_small; // segments of the one-workgroup kernel
    const int* large_list; int n_large;
    const VtTileDev* tile; int n_tile;
    // results per segment (read back once per level)
    unsigned long long* centres;        // [n_seg][k][4]
    int* n_centres; int* iters; int* capped; int* empties;      // [n_seg]
    int* csize;                         // [n_seg][k] members of each final cluster
    // working arrays by position
    unsigned char* assoc; int* min_d;   // [N]
    // multi-workgroup family
    unsigned long long* tile_sum;       // [n_tile]
    unsigned* draw; int* seeding; int* done; int* changed;      // [n_seg]
    unsigned* counters;                 // [n_large][k][256]
    int* members;                       // [n_large][k]
    int* tile_hist;                     // [n_tile][k] counts, then offsets inside the segment
    int* running;                       // [1] a segment has not ended
    int k, max_iterations; unsigned long long seed;
};

size_t vt_small_lds_bytes(int max_n);
hipError_t vt_opt_in_lds();
// every launcher returns the number of kernel launches it made
int vt_launch_small(const VtLevelDev& lv, int max_n, hipStream_t s);
int vt_launch_seed(const VtLevelDev& lv, hipStream_t s);
int vt_launch_iteration(const VtLevelDev& lv, int it, hipStream_t s);          // means (it > 1), assignment, convergence; lv.running[0] != 0 afterwards: go on
int vt_launch_partition(const VtLevelDev& lv, hipStream_t s);
// Ni of features [first, first + n), which belong to images [image_first, image_first + image_count): bitmap [image_count][words32] zeroed by the caller
int vt_launch_count_images(const int32_t* feat_word, const int32_t* offset, int image_first, int image_count, int first, int n, int words32, unsigned* bitmap, int* ni, hipStream_t s);
