// graph_internal.h -- device argument block and launchers of the essential-graph optimisation (graph_kernels.hip / corb_graph.cpp).
#pragma once
#include "corb_internal.h"

struct CorbGraphDev {
    int K, E, nP, sp, fix_scale;
    double* V;                    // [K][8]
    const unsigned char* fixed;   // [K]
    const int* idx;               // [K] hessian index or -1
    const int* vi; const int* vj; // [E]
    const double* meas;           // [E][8]
    double* H; double* A; double* b; double* x;
    double* partial;              // block partial sums
    // deterministic accumulation of the normal equations: the edge kernel stores its Jacobians and error, then one wavefront per free vertex
    // (diagonal block + right-hand side) and one per connected vertex pair (off-diagonal block) sum their edges in edge order
    double* ejac;                 // [E][105] J_i (49, row-major [r][dof]), J_j (49), error (7)
    const int* voff; const int* vedge;            // [nP+1], [.] incident edges of free vertex h: edge id << 1 | role (0 = vertex i of the edge)
    int n_pairs; const int* poff; const int* pedge;   // [n_pairs+1], [.] edges of pair g: edge id << 1 | flipped (edge's (i, j) is the pair's (hi, lo))
    const int* plo; const int* phi;               // [n_pairs] hessian indices lo < hi
};

void eg_launch_chi2(const CorbGraphDev& d, int nparts, double* out, hipStream_t s);
void eg_launch_build(const CorbGraphDev& d, hipStream_t s);
void eg_launch_lambda(const CorbGraphDev& d, double lambda, hipStream_t s);
void eg_launch_update(const CorbGraphDev& d, double lambda, double* scale_out, hipStream_t s);
void eg_launch_apply(int K, const double* S_old, const double* S_new, float* Tiw, int M, const int* ref, float* points, hipStream_t s);

// ---- host side shared by the two entries of the optimisation (corb_graph.cpp): corb_optimize_essential_graph on host arrays, corb_essential_graph_store on the arrays
// its plan left on the device.  Both run on a CorbScratch (lane 1) the caller holds ----
struct CorbScratch;
struct EgSystem { double* Vbak; double* scal; int* info; double* chol_ws; int nparts; };
// hessian index per vertex (-1: fixed) -> idx [K]; returns the number of free vertices
int eg_free_index(int K, const unsigned char* fixed, int* idx);
// refuses a dense system beyond the 200 GB guard (CORB_ERR_ARG with the message set)
int eg_check_size(const char* who, int nP);
// the normal equations, the solver's scalars and the dense solve's workspace for d.K / d.E / d.nP / d.sp
int eg_alloc_system(CorbScratch& pool, CorbGraphDev& d, EgSystem& sys);
// the accumulation lists of the (fixed) graph from host copies of fixed / idx / vi / vj, uploaded; allocates d.ejac
int eg_build_lists(CorbScratch& pool, CorbGraphDev& d, const unsigned char* fixed, const int* idx, const int* vi, const int* vj);
// g2o's Levenberg loop with setUserLambdaInit(1e-16) on d.V; chi2_hist (optional): iterations + 1 doubles
int eg_levenberg(CorbScratch& pool, const CorbGraphDev& d, const EgSystem& sys, int iterations, double* chi2_hist, int* iters_done);
