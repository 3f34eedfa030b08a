// init_kernels.hip -- the monocular Initializer (C/src/Initializer.cc) for gfx950:
//   init_hypothesis_kernel : one single-wave workgroup per (iteration, model, problem): the 8 draws (:87-96), ComputeH21 (:226-266) or ComputeF21 (:268-303) on them
//                            -- the 16 x 9 or 8 x 9 system and V in LDS in FP64, a Jacobi rotation's rows one per lane --, the de-normalisation (:160, :212), then
//                            CheckHomography (:305-388) or CheckFundamental (:390-468) with the lanes striding over the matches: the inlier bits leave through a ballot,
//                            one mask word per 64 matches, and the score is summed by one lane in ascending match order from the terms in LDS (the order is part of
//                            the definition: the score decides which hypothesis wins)
//   init_select_kernel     : one wavefront per problem: the first maximum of the positive scores per model, RH and the model (:112-118), the winners' inlier flags,
//                            then DecomposeE (:909-929) or the 8 hypotheses of Faugeras (:584-686), or an early status
//   init_checkrt_kernel    : one workgroup per (motion hypothesis, problem): one lane per inlier match -- Triangulate's 4 x 4 Jacobi in registers and the tests of
//                            :841-893 --, nGood by an LDS counter, the cosine order statistic of :898-900 by rank counting
//   init_decide_kernel     : one workgroup per problem: :499-569 or :689-731 against the cosine thresholds of the host, then vP3D and vbTriangulated of the winner
// The arithmetic is csrc/init_math.h, the same text a host program runs: the source's float expressions unfused (-ffp-contract=off), decompositions in FP64.
// Compiler's resource summary (hipcc -O3, gfx950):
//   kernel                    VGPRs  SGPRs  scratch bytes  LDS bytes
//   init_hypothesis_kernel       72     53              0       2640
//   init_select_kernel          124     47              0       3072
//   init_checkrt_kernel         146     64              0          4
//   init_decide_kernel           12     46              0         12
#include "init_internal.h"

namespace {

__global__ __launch_bounds__(64) void init_hypothesis_kernel(InitDev d)
{
    __shared__ InitHypWork W;
    init_hypothesis_body(d, blockIdx.y, blockIdx.x >> 1, blockIdx.x & 1, W);
}

__global__ __launch_bounds__(64) void init_select_kernel(InitDev d)
{
    __shared__ InitSelWork W;
    init_select_body(d, blockIdx.x, W);
}

__global__ __launch_bounds__(256) void init_checkrt_kernel(InitDev d)
{
    __shared__ InitRtWork W;
    init_checkrt_body(d, blockIdx.y, blockIdx.x, W);
}

__global__ __launch_bounds__(256) void init_decide_kernel(InitDev d)
{
    __shared__ InitDecWork W;
    init_decide_body(d, blockIdx.x, W);
}

}  // namespace

void corb_launch_mono_initialize(const InitDev& d, hipStream_t s)
{
    if (d.n_problems <= 0) return;
    hipLaunchKernelGGL(init_hypothesis_kernel, dim3(2 * d.max_iterations, d.n_problems), dim3(64), 0, s, d);
    hipLaunchKernelGGL(init_select_kernel, dim3(d.n_problems), dim3(64), 0, s, d);
    hipLaunchKernelGGL(init_checkrt_kernel, dim3(8, d.n_problems), dim3(256), 0, s, d);
    hipLaunchKernelGGL(init_decide_kernel, dim3(d.n_problems), dim3(256), 0, s, d);
}
