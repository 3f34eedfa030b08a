// ba_flatten_dev.cpp -- the host steps around the device flattening (ba_flatten.hip) that its two drivers share: corb_ba_solve_device (corb_ba.cpp: maps) and
// ba_staged_window (corb_ba_staged.cpp: local windows).  What differs between the two on purpose stays with them: one fused scan or four, the counts as one block
// or four copies, pcnt / pcur, the aggregated list kernels, the block pattern.  The pool hands out addresses in call order: the order of the allocations below and
// around the calls is part of the measured layout.
#include "ba_host.h"
#include <algorithm>

// the problem, the per-point / per-keyframe scratch of the first pass, and that pass (active edges per point, hessian flags, edge counts)
int ba_flat_dev_begin(BAFlattenDev& d, const CorbBADeviceProblem* dp, Pool& pool, int** scan_tmp)
{
    const int K = dp->n_poses, M = dp->n_points;
    hipStream_t s = pool.stream;
    memset(&d, 0, sizeof(d));
    d.K = K; d.M = M; d.E = dp->n_edges;
    d.poses = dp->poses; d.pose_fixed = dp->pose_fixed; d.points = dp->points; d.point_fixed = dp->point_fixed; d.edges = dp->edges; d.intr = dp->intr; d.edge_off = dp->edge_off;
    HIPCHK(pool.alloc(&d.lflag, (size_t)M + 1)); HIPCHK(pool.alloc(&d.cntA, (size_t)M + 1)); HIPCHK(pool.alloc(&d.cntB, (size_t)M + 1)); HIPCHK(pool.alloc(&d.nfree_pt, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.lidx, (size_t)M + 1)); HIPCHK(pool.alloc(&d.eoffA, (size_t)M + 1)); HIPCHK(pool.alloc(&d.eoffB, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.pflag, (size_t)K + 1)); HIPCHK(pool.alloc(&d.pidx, (size_t)K + 1)); HIPCHK(pool.alloc(&d.pt_touched, (size_t)M + 1));
    HIPCHK(pool.alloc(&d.scal, FLAT_NSCAL));
    HIPCHK(pool.alloc(scan_tmp, corb_scan_scratch_ints((size_t)std::max(std::max(K, M), 1))));
    HIPCHK(hipMemsetAsync(d.scal, 0, sizeof(int) * FLAT_NSCAL, s));
    flat_launch_points(d, s);
    return CORB_OK;
}
// hessian indices of the points and keyframes, edge offsets of the two edge groups: four scans
void ba_flat_dev_scans(const BAFlattenDev& d, int* scan_tmp, hipStream_t s)
{
    corb_launch_exclusive_scan(d.lflag, d.lidx, (size_t)d.M, scan_tmp, s);
    corb_launch_exclusive_scan(d.cntA, d.eoffA, (size_t)d.M, scan_tmp, s);
    corb_launch_exclusive_scan(d.cntB, d.eoffB, (size_t)d.M, scan_tmp, s);
    corb_launch_exclusive_scan(d.pflag, d.pidx, (size_t)d.K, scan_tmp, s);
}
// the estimates and the sorted structure-of-arrays edges, landmark ranges and vertex tables of a BAFlat whose counts are known (with_e_src: the window route's map
// back to the problem's edges, between the edge arrays and the ranges)
int ba_flat_dev_alloc(BAFlattenDev& d, BAFlat& f, Pool& pool, bool with_e_src)
{
    const size_t nE = (size_t)f.nE, nP = (size_t)f.nP, nL = (size_t)f.nL;
    f.n_q = 4 * (size_t)d.K; f.n_t = 3 * (size_t)d.K; f.n_pt = 3 * (size_t)d.M;
    HIPCHK(pool.alloc(&f.dq, f.n_state())); HIPCHK(pool.alloc(&f.dq_bak, f.n_state()));
    HIPCHK(pool.alloc(&f.e_pose, nE)); HIPCHK(pool.alloc(&f.e_point, nE)); HIPCHK(pool.alloc(&f.e_vpose, nE)); HIPCHK(pool.alloc(&f.e_vpoint, nE));
    HIPCHK(pool.alloc(&f.e_obs, 3 * nE)); HIPCHK(pool.alloc(&f.e_w, nE)); HIPCHK(pool.alloc(&f.e_dim, nE)); if (with_e_src) HIPCHK(pool.alloc(&d.e_src, nE));
    HIPCHK(pool.alloc(&f.loff, nL + 1)); HIPCHK(pool.alloc(&f.lnfree, nL + 1)); HIPCHK(pool.alloc(&f.poff, nP + 1));
    HIPCHK(pool.alloc(&f.pose_vertex, nP + 1)); HIPCHK(pool.alloc(&f.point_vertex, nL + 1)); HIPCHK(pool.alloc(&f.cam, 5 * (size_t)std::max(d.K, 1)));
    return CORB_OK;
}
// ... cleared where the edge pass counts, and handed to the flattening's kernels
int ba_flat_dev_wire(BAFlattenDev& d, BAFlat& f, Pool& pool)
{
    HIPCHK(hipMemsetAsync(f.loff, 0, sizeof(int) * ((size_t)f.nL + 1), pool.stream));
    d.e_pose = f.e_pose; d.e_point = f.e_point; d.e_vpose = f.e_vpose; d.e_vpoint = f.e_vpoint; d.e_obs = f.e_obs; d.e_w = f.e_w; d.e_dim = f.e_dim;
    d.loff = f.loff; d.lnfree = f.lnfree; d.poff = f.poff; d.pose_vertex = f.pose_vertex; d.point_vertex = f.point_vertex; d.cam = f.cam; d.state = f.dq;
    return CORB_OK;
}
