// corb_newpoints.cpp -- C-ABI host side of LocalMapping::CreateNewMapPoints (include/corb_accel.h, last section): the host-array form for adapters
// (corb_triangulate_pairs: the pairs of one SearchForTriangulation call) and the whole neighbour loop on records (corb_create_new_map_points_store: matching,
// triangulation and the new MapPoint records with one synchronisation and one read-back).
#include "newpoints_internal.h"
#include "match_internal.h"
#include "record_call.h"
#include <cstring>
#include <vector>

namespace {
bool side_ok(const CorbNewPointSide* s)
{
    return s && s->n >= 0 && s->nlevels >= 1 && s->nlevels <= CORB_MAX_LEVELS && s->scale && (s->n == 0 || (s->keys_un && s->u_right && s->depth));
}
void side_values(NpSide& d, const CorbNewPointSide* s)
{
    memcpy(d.Tcw, s->Tcw, sizeof(d.Tcw)); d.hdr = nullptr;
    d.fx = s->fx; d.fy = s->fy; d.cx = s->cx; d.cy = s->cy; d.bf = s->bf; d.mb = s->mb; d.nlevels = s->nlevels;
    for (int l = 0; l < CORB_MAX_LEVELS; l++) d.scale[l] = l < s->nlevels ? s->scale[l] : 1.f;
}
void side_record(NpSide& d, const char* rec, const RecLayout& L, const CorbTrackCamera* cam)
{
    memset(&d, 0, sizeof(d));
    d.kp = reinterpret_cast<const CorbKeyPoint*>(rec + L.kp); d.ur = reinterpret_cast<const float*>(rec + L.ur); d.depth = reinterpret_cast<const float*>(rec + L.depth);
    d.hdr = reinterpret_cast<const KfHeader*>(rec);
    d.mb = cam->mb; d.nlevels = cam->nlevels;
    for (int l = 0; l < CORB_MAX_LEVELS; l++) d.scale[l] = l < cam->nlevels ? cam->scale[l] : 1.f;
}
}  // namespace

extern "C" int corb_triangulate_pairs(const CorbNewPointSide* kf1, const CorbNewPointSide* kf2, const int32_t* pairs, int n_pairs,
                                      float* x3d, uint8_t* status, uint8_t* source, int* n_new, int device)
{
    const char* who = "corb_triangulate_pairs";
    if (!side_ok(kf1) || !side_ok(kf2) || n_pairs < 0 || !n_new || (n_pairs > 0 && (!pairs || !x3d || !status || !source))) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    for (int i = 0; i < n_pairs; i++)
        if (pairs[2 * i] < 0 || pairs[2 * i] >= kf1->n || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= kf2->n) { corb_set_error("%s: pair %d names a feature out of range", who, i); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    *n_new = 0;
    if (n_pairs == 0) return CORB_OK;
    CorbScratch pool(0);
    NpDev d; memset(&d, 0, sizeof(d));
    side_values(d.s1, kf1); side_values(d.s2, kf2);
    const size_t n1 = (size_t)kf1->n, n2 = (size_t)kf2->n;
    HIPCHK(pool.upload_block({{(void**)&d.s1.kp, kf1->keys_un, n1 * 28}, {(void**)&d.s1.ur, kf1->u_right, n1 * 4}, {(void**)&d.s1.depth, kf1->depth, n1 * 4},
                              {(void**)&d.s2.kp, kf2->keys_un, n2 * 28}, {(void**)&d.s2.ur, kf2->u_right, n2 * 4}, {(void**)&d.s2.depth, kf2->depth, n2 * 4},
                              {(void**)&d.pairs, pairs, (size_t)n_pairs * 8}}));
    d.n = n_pairs; d.n2 = kf2->n;
    HIPCHK(pool.alloc(&d.x3d, (size_t)n_pairs * 3)); HIPCHK(pool.alloc(&d.status, (size_t)n_pairs)); HIPCHK(pool.alloc(&d.source, (size_t)n_pairs)); HIPCHK(pool.alloc(&d.n_new, 1));
    HIPCHK(hipMemsetAsync(d.n_new, 0, 4, pool.stream));
    corb_launch_newpoints(d, pool.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(pool.d2h(x3d, d.x3d, (size_t)n_pairs * 12)); HIPCHK(pool.d2h(status, d.status, (size_t)n_pairs)); HIPCHK(pool.d2h(source, d.source, (size_t)n_pairs));
    HIPCHK(pool.d2h(n_new, d.n_new, 4));
    HIPCHK(pool.fetch_finish());
    return CORB_OK;
}

extern "C" int corb_create_new_map_points_store(CorbKfStore* kf, int cur_slot, const int32_t* nb_slots, int n_nb, const float* F12, const float* epipole,
                                                const CorbTrackCamera* cam, int only_stereo, int apply, CorbMpStore* map, int first_mp_slot, uint64_t first_mp_id,
                                                int32_t client_id, int32_t* pair_offset, int32_t* pairs, float* x3d, uint8_t* status, uint8_t* source, int* n_new)
{
    const char* who = "corb_create_new_map_points_store";
    if (!kf || !cam || cur_slot < 0 || cur_slot >= kf->capacity || n_nb < 0 || !pair_offset || !n_new || (n_nb > 0 && (!nb_slots || !F12 || !epipole)) ||
        cam->nlevels < 1 || cam->nlevels > CORB_MAX_LEVELS) { corb_set_error("%s: bad argument", who); return CORB_ERR_ARG; }
    for (int j = 0; j < n_nb; j++) {
        bool ok = nb_slots[j] >= 0 && nb_slots[j] < kf->capacity && nb_slots[j] != cur_slot;
        for (int i = 0; i < j && ok; i++) ok = nb_slots[i] != nb_slots[j];
        if (!ok) { corb_set_error("%s: neighbour %d: slot out of range, the current keyframe's, or named twice", who, j); return CORB_ERR_ARG; }
    }
    if (apply && (!map || map->device != kf->device || first_mp_slot < 0 || first_mp_slot > map->capacity)) { corb_set_error("%s: bad map-point store / first slot", who); return CORB_ERR_ARG; }
    if (apply && map->O < 2) { corb_set_error("%s: the map-point store holds fewer than two observations per point", who); return CORB_ERR_CAPACITY; }
    int rc = corb_select_device(kf->device); if (rc) return rc;
    RecordCall call; call.hold(nullptr, kf, nullptr, apply ? map : nullptr);            // (the map is written only when the points are applied)
    const CorbKfStore::Host& hc = kf->host[cur_slot];
    if (record_slot_count(who, kf, cur_slot, true) < 0) return CORB_ERR_ARG;
    for (int j = 0; j < n_nb; j++) if (kf->host[nb_slots[j]].n < 0 || !kf->host[nb_slots[j]].header_valid) { corb_set_error("%s: neighbour slot %d is empty", who, nb_slots[j]); return CORB_ERR_ARG; }
    const int n1 = hc.n;
    for (int j = 0; j <= n_nb; j++) pair_offset[j] = 0;
    *n_new = 0;
    if (n_nb == 0 || n1 == 0) return CORB_OK;
    if (!pairs || !x3d || !status || !source) { corb_set_error("%s: NULL output", who); return CORB_ERR_ARG; }
    rc = call.join(); if (rc) return rc;

    // the common vocabulary nodes of every neighbour, from the host mirror of the node ids
    std::vector<int> pa, pb, com_off((size_t)n_nb + 1, 0);
    for (int j = 0; j < n_nb; j++) { common_nodes(hc.node_id, kf->host[nb_slots[j]].node_id, pa, pb); com_off[(size_t)j + 1] = (int)pa.size(); }
    const size_t total = (size_t)n_nb * n1, F = (size_t)kf->F;
    float sigma2[CORB_MAX_LEVELS];
    for (int l = 0; l < cam->nlevels; l++) sigma2[l] = cam->scale[l] * cam->scale[l];                   // mvLevelSigma2 (ORBextractor.cc:418-430)
    CorbScratch pool(0);
    int *dpa, *dpb, *dslots; float *dsc, *dsg;
    HIPCHK(pool.upload_block({{(void**)&dpa, pa.data(), pa.size() * 4}, {(void**)&dpb, pb.data(), pb.size() * 4}, {(void**)&dslots, nb_slots, (size_t)n_nb * 4},
                              {(void**)&dsc, cam->scale, (size_t)cam->nlevels * 4}, {(void**)&dsg, sigma2, (size_t)cam->nlevels * 4}}));
    // [match | winner] = -1 and status = CORB_NP_NONE in one fill; the counters (per neighbour: matches, queries; then n_new; then the two totals) in another
    int* dmatch; HIPCHK(pool.alloc(&dmatch, total + (size_t)n_nb * F + (total + 3) / 4));
    int* dwinner = dmatch + total; unsigned char* dstatus = reinterpret_cast<unsigned char*>(dwinner + (size_t)n_nb * F);
    HIPCHK(hipMemsetAsync(dmatch, 0xFF, (total + (size_t)n_nb * F) * 4 + total, pool.stream));
    int* dcnt; HIPCHK(pool.alloc(&dcnt, 2 * (size_t)n_nb + 3));
    HIPCHK(hipMemsetAsync(dcnt, 0, (2 * (size_t)n_nb + 3) * 4, pool.stream));
    int* dn_new = dcnt + 2 * (size_t)n_nb; int* dtotals = dn_new + 1;
    float* dx3d; unsigned char *dsource, *dflags; int *dq1, *dq2, *drank;
    HIPCHK(pool.alloc(&dx3d, total * 3)); HIPCHK(pool.alloc(&dsource, total)); HIPCHK(pool.alloc(&dflags, (size_t)n1)); HIPCHK(pool.alloc(&dq1, (size_t)n1)); HIPCHK(pool.alloc(&dq2, (size_t)n1));
    HIPCHK(pool.alloc(&drank, total));
    HIPCHK(hipMemsetAsync(dx3d, 0, total * 12, pool.stream)); HIPCHK(hipMemsetAsync(dsource, 0, total, pool.stream));
    const char* rc1 = kf->rec(cur_slot); const RecLayout& L = kf->L;
    HIPCHK(hipMemcpyAsync(dflags, rc1 + L.flags, (size_t)n1, hipMemcpyDeviceToDevice, pool.stream));      // the evolving flags live in call scratch

    for (int j = 0; j < n_nb; j++) {
        const int n_common = com_off[(size_t)j + 1] - com_off[j], n2 = kf->host[nb_slots[j]].n;
        if (n_common == 0 || n2 == 0) continue;
        const char* rc2 = kf->rec(nb_slots[j]);
        int* dm = dmatch + (size_t)j * n1; int* dnm = dcnt + 2 * (size_t)j; int* dnq = dnm + 1;
        corb_launch_tri_queries((const int*)(rc1 + L.fv_off), (const int*)(rc1 + L.fv_idx), dflags, (const float*)(rc1 + L.ur), dpa + com_off[j], dpb + com_off[j], n_common,
                                only_stereo ? 1 : 0, dq1, dq2, dnq, pool.stream);
        CorbTriDev t; memset(&t, 0, sizeof(t));
        t.n_queries = n1; t.n_queries_dev = dnq; t.only_stereo = only_stereo ? 1 : 0; t.check_ori = 0;      // ORBmatcher(0.6, false)
        t.q_idx1 = dq1; t.q_node2 = dq2; t.off2 = (const int*)(rc2 + L.fv_off); t.idx2 = (const int*)(rc2 + L.fv_idx);
        t.desc1 = (const unsigned long long*)(rc1 + L.desc); t.desc2 = (const unsigned long long*)(rc2 + L.desc);
        t.kp1 = (const CorbKeyPoint*)(rc1 + L.kp); t.kp2 = (const CorbKeyPoint*)(rc2 + L.kp);
        t.uright1 = (const float*)(rc1 + L.ur); t.uright2 = (const float*)(rc2 + L.ur); t.has_mp2 = (const uint8_t*)(rc2 + L.flags);
        for (int i = 0; i < 9; i++) t.F12[i] = F12[9 * (size_t)j + i];
        t.ex = epipole[2 * (size_t)j]; t.ey = epipole[2 * (size_t)j + 1]; t.scale2 = dsc; t.sigma2_2 = dsg;
        t.match = dm; t.bin = nullptr; t.hist = nullptr; t.n_matches = dnm;
        corb_launch_tri(t, n1, pool.stream);
        NpDev d; memset(&d, 0, sizeof(d));
        side_record(d.s1, rc1, L, cam); side_record(d.s2, rc2, L, cam);
        d.match = dm; d.n = n1; d.n2 = n2;
        d.x3d = dx3d + 3 * (size_t)j * n1; d.status = dstatus + (size_t)j * n1; d.source = dsource + (size_t)j * n1;
        d.flags1 = dflags; d.winner = dwinner + (size_t)j * F; d.n_new = dn_new;
        corb_launch_newpoints(d, pool.stream);
    }
    NpApplyDev a; memset(&a, 0, sizeof(a));
    a.n_nb = n_nb; a.n1 = n1; a.apply = apply ? 1 : 0; a.match = dmatch; a.x3d = dx3d; a.status = dstatus; a.winner = dwinner; a.rank = drank; a.totals = dtotals;
    a.kf_base = kf->base(); a.kf_bytes = L.bytes; a.F = kf->F; a.cur_slot = cur_slot; a.nb_slots = dslots;
    if (apply) { a.mp_base = map->base(); a.mp_bytes = map->L.bytes; a.max_obs = map->O; a.mp_capacity = map->capacity; a.first_mp_slot = first_mp_slot; a.first_mp_id = first_mp_id; a.client_id = client_id; }
    a.nlevels = cam->nlevels; for (int l = 0; l < CORB_MAX_LEVELS; l++) a.scale[l] = l < cam->nlevels ? cam->scale[l] : 1.f;
    corb_launch_newpoints_apply(a, pool.stream);
    HIPCHK(hipGetLastError());

    static thread_local std::vector<int> h_match; static thread_local std::vector<float> h_x3d; static thread_local std::vector<unsigned char> h_st, h_src;
    h_match.resize(total); h_x3d.resize(total * 3); h_st.resize(total); h_src.resize(total);
    int h_tot[2] = {0, 0};
    HIPCHK(pool.d2h(h_match.data(), dmatch, total * 4)); HIPCHK(pool.d2h(h_x3d.data(), dx3d, total * 12)); HIPCHK(pool.d2h(h_st.data(), dstatus, total));
    HIPCHK(pool.d2h(h_src.data(), dsource, total)); HIPCHK(pool.d2h(h_tot, dtotals, 8));
    HIPCHK(pool.fetch_finish());
    int k = 0;
    for (int j = 0; j < n_nb; j++) {
        pair_offset[j] = k;
        for (int i = 0; i < n1; i++) {
            const size_t e = (size_t)j * n1 + i;
            if (h_st[e] == CORB_NP_NONE) continue;
            pairs[2 * k] = i; pairs[2 * k + 1] = h_match[e];
            x3d[3 * k] = h_x3d[3 * e]; x3d[3 * k + 1] = h_x3d[3 * e + 1]; x3d[3 * k + 2] = h_x3d[3 * e + 2];
            status[k] = h_st[e]; source[k] = h_src[e]; k++;
        }
    }
    pair_offset[n_nb] = k;
    *n_new = h_tot[0];
    if (apply && h_tot[1]) { corb_set_error("%s: %d new map points, the store has room for %d from slot %d; no record was written", who, h_tot[0], map->capacity - first_mp_slot, first_mp_slot); return CORB_ERR_CAPACITY; }
    if (apply && h_tot[0] > 0) map->idt_valid = false;          // the slots hold other ids now: corb_mp_store_build_index again before the tracking calls
    return CORB_OK;
}
