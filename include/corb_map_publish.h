/* corb_map_publish.h -- the server -> clients direction of the record path: what MapFusion::runPubTopic (S/src/MapFusion.cpp:315-368) and resentGlobalMapToClient
 * (:370-430) hand to PubToClient (S/src/PubToClient.cpp:24-163) and every client's Cache files in its four subscriber callbacks (C/src/Cache.cc:446-634), on
 * device-resident records.  Exported from libcorb_accel.so beside the drop-in boundary of corb_accel.h.
 *
 * The calls take no workspace lane.  Their temporaries belong to a handle, CorbMapPublisher, created once per rank: one stream, a page-locked staging block, the
 * device message buffer, a receive buffer and all scratch.  Buffers grow on demand and are never freed per call; every buffer is written by a call before that
 * call reads it, so a call's outputs do not depend on what the handle served before (WORKSPACE_AUDIT.md).  A handle serves one call at a time (it locks itself).
 *
 * House rules as for the other calls on records: argument errors are a status with a message in corb_last_error(); the handle, then the keyframe store, then the
 * map-point store are locked before a count is read; one synchronisation and one read-back per call; the decisions are computed from the records as they stand
 * before the call and from the message, so apply == 0 reports exactly what apply != 0 does; on CORB_ERR_CAPACITY nothing is written and the outputs are complete.
 * The definition of every output, every message byte and every record byte is tests/publish_reference.py.
 *
 * The message: ONE contiguous device buffer of five sections, each starting at a multiple of 16 bytes (corb_pub_message_layout); the counts travel beside it.
 *   A  counts[0] whole keyframe records (corb_kf_store_record_bytes each)       the new keyframes            (PubToClient::pubNewKFsToClients)
 *   B  counts[1] whole map-point records (corb_mp_store_record_bytes each)      the new map points           (pubNewMPsToClients)
 *   C  counts[2] CorbKeyFramePosePacket                                          the updated keyframe poses   (pubUpdatedKFsToClients; KeyFramePose, C/src/TransPose.cpp:13-18)
 *   D  counts[3] CorbMapPointPosePacket                                          the updated positions        (pubUpdatedMPsToClients; MapPointPose)
 *   E  counts[4] CorbPublishTransform                                            PubToClient::transMs: per client its frame's transform T and T^-1
 * Entries keep the order of the caller's slot lists (the adapter passes ascending id, as std::set<LightKeyFrame> iterates). */
#ifndef CORB_MAP_PUBLISH_H
#define CORB_MAP_PUBLISH_H
#include "corb_accel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct CorbKeyFramePosePacket { uint64_t id; float Tcw[16]; } CorbKeyFramePosePacket;                        /* 72 bytes */
typedef struct CorbMapPointPosePacket { uint64_t id; float pos[3]; uint32_t pad; } CorbMapPointPosePacket;           /* 24 bytes, pad = 0 */
typedef struct CorbPublishTransform { int32_t client_id; int32_t pad; float T[16]; float Tinv[16]; } CorbPublishTransform;      /* 136 bytes, row-major 4x4 */

typedef struct CorbMapPublisher CorbMapPublisher;
int corb_pub_create(int device, CorbMapPublisher** out);
void corb_pub_destroy(CorbMapPublisher* h);

/* offsets[0..4] = byte offset of sections A..E, offsets[5] = the message's size, for these counts and record sizes.  Pure arithmetic; CORB_ERR_ARG on a negative
 * count, a record size that is not a positive multiple of 16 where its count is non-zero, or a message of 2^31 bytes or more (a message is one transfer). */
int corb_pub_message_layout(const int32_t counts[5], int kf_record_bytes, int mp_record_bytes, int64_t offsets[6]);

/* Server side.  Gathers the five sections into the handle's message buffer under the stores' locks: A / B the whole records of new_kf_slots / new_mp_slots, C / D
 * the id and Tcw / world_pos of the record headers of upd_kf_slots / upd_mp_slots, E the table: entry k = {trans_client_id[k], trans[16 k ..], its inverse}.
 * The inverse is computed once per entry on the host (csrc/publish_math.h): cv::Mat::inv of a float 4x4 read as the cofactor inverse of the FULL 4x4 in double
 * from the float entries, times 1 / det, each entry rounded to float once -- the general inverse, not the rigid one (a monocular To2n carries a scale).
 * CORB_ERR_ARG, and nothing packed (the message the handle held stays): a keyframe slot that is empty, any slot out of range, a client id named twice, a table
 * entry whose determinant is zero or not finite.  kf / mp may be NULL when their two lists are empty.  All sections empty is a valid (empty) message. */
int corb_pub_pack(CorbMapPublisher* h, CorbKfStore* kf, const int32_t* new_kf_slots, int n_new_kf, const int32_t* upd_kf_slots, int n_upd_kf,
                  CorbMpStore* mp, const int32_t* new_mp_slots, int n_new_mp, const int32_t* upd_mp_slots, int n_upd_mp,
                  const int32_t* trans_client_id, const float* trans, int n_trans);
/* the message of the last successful pack: device address (NULL for an empty one), size, counts and the record sizes it was packed with (any output may be NULL) */
int corb_pub_message(CorbMapPublisher* h, void** device_ptr, int64_t* bytes, int32_t counts[5], int32_t* kf_record_bytes, int32_t* mp_record_bytes);
/* the message's bytes on the host (tests, tools); cap < its size: CORB_ERR_CAPACITY */
int corb_pub_message_read(CorbMapPublisher* h, void* host, int64_t cap);

/* What corb_pub_apply and the receiving side of corb_map_publish return.  The arrays are the caller's, with room for counts[0], [1], [2], [3] entries (kind_*)
 * and min(counts[0], kf_room) / min(counts[1], mp_room) entries (the slot lists); any of them may be NULL. */
typedef struct CorbPublishOutputs {
    uint8_t* kind_kf_new; uint8_t* kind_mp_new; uint8_t* kind_kf_upd; uint8_t* kind_mp_upd;
    int32_t* kf_new_slots; int32_t* mp_new_slots;              /* the slot the k-th accepted entry went to (would go to): free_first + k */
    int32_t n_kf_inserted, n_mp_inserted;                      /* entries of kind 3 in A / B */
    int32_t n_kf_updated, n_mp_updated;                        /* entries of kind 2 in C / D */
    int32_t no_transform;                                      /* 1: client_id is not in section E -- nothing applies, every kind is 0 */
} CorbPublishOutputs;

/* Client side.  msg: a device pointer to a message with these counts and record sizes (another handle's, or what corb_map_publish received), on the handle's
 * device.  The four phases run in the reference's publication order (MapFusion.cpp:352-358): A, B, C, D; every phase sees what the earlier phases of the same call
 * wrote.  Keyframe ids resolve over the slots [kf_first, kf_first + kf_n) of dst_kf through an id table the call builds (a slot without features is not a
 * keyframe, of two slots with one id the lower is the keyframe -- as corb_mp_store_replace finds them); map-point ids through dst_mp's id index, which must be
 * current on entry and cover exactly [mp_first, mp_first + mp_n) (corb_mp_store_build_index).  Bad flags are consulted nowhere, as getKeyFrameById /
 * getMapPointById do not look at them.
 *   no transform  client_id is in no entry of E (the `return` at Cache.cc:456, :504, :555, :599): nothing is applied, every kind is 0, no_transform = 1.
 *   A (Cache.cc:465-489)  kind_kf_new[i]: 1 the record's client_id equals client_id, skipped; 2 its id is already held, skipped; 3 accepted.  Of several entries
 *     with one id the LOWEST position is 3 and the others are 2 (the serial loop in closed form: getKeyFrameById is true by then).  The k-th accepted entry in
 *     message order becomes slot kf_free_first + k: the whole record is copied, then Tcw <- Tcw * Tinv in the arithmetic of corb_rebase_map_store (exact products
 *     summed in double, left to right, one rounding, all 16 entries) and flags |= CORB_KF_FIXED; TcwGBA and everything else as sent.  The store's host mirror of
 *     the slot (feature count, id, header validity) is made current.  More accepted entries than kf_room: CORB_ERR_CAPACITY, no phase writes anything.
 *   B (:515-540)  the same three kinds on map points; world_pos <- R p + t with R, t of T (not Tinv) as one gemm row: the double row sum plus (double)t, rounded
 *     once; flags |= CORB_MP_FIXED.  The observations travel with the record.  normal, min_distance and max_distance travel UNCHANGED: the reference neither
 *     rotates mNormalVector nor calls UpdateNormalAndDepth here, and this call keeps that.  The k-th accepted entry becomes slot mp_free_first + k;
 *     with a non-empty B, mp_free_first must be mp_first + mp_n (the id index covers one run of slots).  If any entry was accepted the call rebuilds the id index
 *     over [mp_first, mp_first + mp_n + n_mp_inserted) and leaves it current.
 *   C (:566-583)  kind_kf_upd[i]: 0 id not held; 1 held but not CORB_KF_FIXED, left alone (a client's own keyframes are never moved by the server); 2 Tcw <-
 *     KFPose * Tinv.  A keyframe phase A of this call accepted is held and fixed.  Of several entries with one id the HIGHEST position's value stays.
 *   D (:610-630)  the same kinds with CORB_MP_FIXED and world_pos <- R p + t.
 * apply == 0 reports exactly what apply != 0 would and writes nothing.  The free slots must not overlap the resolved ranges.
 * Returns CORB_OK, CORB_ERR_ARG, CORB_ERR_CAPACITY (outputs complete, nothing written) or CORB_ERR_HIP. */
int corb_pub_apply(CorbMapPublisher* h, const void* msg, const int32_t counts[5], int kf_record_bytes, int mp_record_bytes, int32_t client_id,
                   CorbKfStore* dst_kf, int kf_first, int kf_n, int kf_free_first, int kf_room,
                   CorbMpStore* dst_mp, int mp_first, int mp_n, int mp_free_first, int mp_room, int apply, CorbPublishOutputs* out);

/* ---- the collective: every rank calls it with its communicator and its own handle; blocking only ---- */
typedef struct CorbPublishPack {          /* the root's arguments = corb_pub_pack's */
    CorbKfStore* kf; const int32_t* new_kf_slots; int32_t n_new_kf; const int32_t* upd_kf_slots; int32_t n_upd_kf;
    CorbMpStore* mp; const int32_t* new_mp_slots; int32_t n_new_mp; const int32_t* upd_mp_slots; int32_t n_upd_mp;
    const int32_t* trans_client_id; const float* trans; int32_t n_trans;
} CorbPublishPack;
typedef struct CorbPublishApply {         /* every other rank's arguments = corb_pub_apply's */
    int32_t client_id;
    CorbKfStore* dst_kf; int32_t kf_first, kf_n, kf_free_first, kf_room;
    CorbMpStore* dst_mp; int32_t mp_first, mp_n, mp_free_first, mp_room;
    int32_t apply;
    CorbPublishOutputs* out;              /* arrays sized for the largest message the caller expects; kind arrays too small cannot be detected: pass NULL to skip one */
} CorbPublishApply;
/* what a rank contributes to the one header all-gather: 8 ints.  counts: the root's only. */
typedef struct CorbPublishHeader { int32_t status, kf_record_bytes, mp_record_bytes, counts[5]; } CorbPublishHeader;
/* The verdict every rank returns before a byte moves, as a pure function of the gathered headers (no device, no communicator): a rank's local status; a negative
 * count of the root's; a receiver whose record size differs from the root's while the matching count (A for keyframes, B for map points) is non-zero =>
 * CORB_ERR_ARG.  *failing_rank = the first rank the verdict is about (-1 if none). */
int corb_map_publish_plan(int world, int root, const CorbPublishHeader* headers /* [world] */, int* failing_rank);
/* The messages of a publish whose plan is CORB_OK: the root SENDS one message of the total size to every other rank, in rank order; every other rank RECEIVES
 * one from the root (kind 0, first_record 0, n_records = the sum of the five counts).  An all-empty message: nothing is exchanged.  sends: room for world entries,
 * recvs: for one. */
int corb_map_publish_messages(int world, int rank, int root, const CorbPublishHeader* headers /* [world] */, CorbPushMsg* sends, int* n_sends, CorbPushMsg* recvs, int* n_recvs);
/* The root passes `pack` (apply_args NULL) and applies nothing; every other rank passes `apply_args` (pack NULL).  One header all-gather, the plan's verdict on
 * every rank, then the root packs and the message travels over the communicator's transport (in-process: device-to-device copies; RCCL: one grouped send /
 * receive), then every receiver applies from its handle's receive buffer.  The verdict is common to all ranks; the APPLY status is per rank: one client's
 * CORB_ERR_CAPACITY does not undo another client's apply, exactly as one subscriber's failure does not in the reference.  A receiver whose destination store is
 * the root's source store is refused (in-process transport, where ranks can share stores): CORB_ERR_ARG for every rank.  With an all-empty message the
 * receivers' outputs are zeros. */
int corb_map_publish(CorbComm* c, CorbMapPublisher* h, int root, const CorbPublishPack* pack, const CorbPublishApply* apply_args);

#ifdef __cplusplus
}
#endif
#endif
