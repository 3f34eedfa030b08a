// init_internal.h -- device-side argument block of the monocular Initializer (init_kernels.hip, corb_initializer.cpp): InitDev of init_math.h
#pragma once
#include "corb_internal.h"
#include "init_math.h"

// hypotheses (one wavefront per problem, iteration and model), select (one per problem), CheckRT (one workgroup per problem and motion hypothesis), decide (one per
// problem).  The candidate arrays, p3d and tri are zero on entry.
void corb_launch_mono_initialize(const InitDev& d, hipStream_t s);
