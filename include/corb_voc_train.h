/* corb_voc_train.h -- vocabulary training and export for libcorb_accel.so: DBoW2's TemplatedVocabulary::create (hierarchical k-means++ on ORB descriptors, TF_IDF weights,
 * L1_NORM scoring) on the device, a vocabulary back as flat arrays, and the reference's text format (saveToTextFile).
 *
 * An offline tool beside the drop-in boundary of corb_accel.h: the SLAM loop never calls it.  The functions are exported from the same library.  A training call takes
 * no workspace lane: it allocates its own device buffers, runs on its own stream and frees everything but the vocabulary before it returns.
 *
 * The definition is tests/voctrain_reference.py (readings of the source: DESIGN.md section 2): random draws are a function of (seed, node path, draw number), so a seed
 * gives one vocabulary whatever the device does in parallel.  Errors follow the house rule: a status, a message in corb_last_error(), nothing written. */
#ifndef CORB_VOC_TRAIN_H
#define CORB_VOC_TRAIN_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CORB_VOC_TRAIN_MAX_LEVELS 10

typedef struct CorbVocTrainOptions {
    int32_t k, L;                 /* branching factor 2 .. 20, depth 1 .. 10 */
    int32_t max_iterations;       /* >= 1: passes of the association step per k-means node, the first included; a node that reaches it is counted as capped */
    int32_t reserved;             /* 0 */
    uint64_t seed;
} CorbVocTrainOptions;

typedef struct CorbVocTrainStats {
    int32_t nodes, words;                      /* of the tree, the root included */
    int32_t kmeans_nodes, trivial_nodes;       /* nodes split by k-means; nodes of n <= k features, one cluster per feature */
    int32_t short_nodes;                       /* k-means nodes that kept fewer than k centres (all remaining distances 0) */
    int32_t max_iterations_seen, capped_nodes;
    int32_t empty_cluster_events;              /* a cluster without members in a later pass: its centre stayed */
    int32_t level_nodes[CORB_VOC_TRAIN_MAX_LEVELS];             /* split nodes per level, [0] the root */
    int32_t level_max_iterations[CORB_VOC_TRAIN_MAX_LEVELS];
    int32_t level_launches[CORB_VOC_TRAIN_MAX_LEVELS];          /* kernel launches per level */
    int32_t level_small_nodes[CORB_VOC_TRAIN_MAX_LEVELS];       /* nodes the one-workgroup kernel took */
    int32_t level_large_nodes[CORB_VOC_TRAIN_MAX_LEVELS];       /* nodes the multi-workgroup kernels took */
    int32_t launches;                          /* all kernel launches of the call, the weights' included */
    int32_t small_limit;                       /* CORB_VOC_TRAIN_SMALL as used */
    double elapsed_ms;                         /* wall clock of the call */
} CorbVocTrainStats;

/* desc = [offset[n_images]][32] descriptors of n_images training images, image i = [offset[i], offset[i + 1]); images may be empty.  *out is an ordinary CorbVoc:
 * every corb_voc_* / corb_kfdb_* call takes it; free it with corb_voc_destroy.  stats is optional. */
int corb_voc_train(const uint8_t* desc, const int32_t* offset, int n_images, const CorbVocTrainOptions* opt, int device, CorbVoc** out, CorbVocTrainStats* stats);

/* the same on keyframe records: every slot is one image, its descriptors are gathered on the device.  A slot given twice: CORB_ERR_ARG. */
int corb_voc_train_store(CorbKfStore* s, const int32_t* slots, int n_slots, const CorbVocTrainOptions* opt, CorbVoc** out, CorbVocTrainStats* stats);

/* CorbVocDesc's arrays of any vocabulary (node ids 1 .. *n_nodes in array order).  More than cap_nodes: CORB_ERR_OVERFLOW with *n_nodes set, nothing written. */
int corb_voc_get(const CorbVoc* v, int32_t* parent, int32_t* is_leaf, uint8_t* descriptor, double* weight, int cap_nodes, int* n_nodes);

/* saveToTextFile.  weight_digits 0: the reference's bytes (header `k L  0 0`, a space after every descriptor byte, weights as %g); 1 .. 17: weights as %.{digits}g --
 * 17 gives a file that reloads bit for bit. */
int corb_voc_save_text(const CorbVoc* v, const char* path, int weight_digits);

#ifdef __cplusplus
}
#endif
#endif
